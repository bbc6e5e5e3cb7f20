"""The needle lengths at which private search changes shape, one text that holds a needle of every
such length, and the shape of a find's schedule derived from the chunking rule alone: shared by
tests/test_private_needle.py, tests/test_find_clear.py and tests/test_scan_clear.py on the CPU and
tests/test_needle_limits_gpu.py on the device.  No GPU use, no test functions
(tests/selector_cases.py is the precedent); the helpers of other test modules are imported inside
the functions, since those modules import this one.

2 m nibble tests are cut into balanced chunks of at most 16 (lower.h for_balanced_chunks):
  m =  8: 16 tests, one chunk of 16 (the widest sum a sign gate reads: offset -31);
  m = 16: 16 + 16;  m = 17: 12 + 11 + 11, the first three unequal chunks;  m = 32: four of 16;
  m = 33: 14 + 13 + 13 + 13 + 13;  m = 63: six of 16 and two of 15;  m = 64: eight of 16, the limit."""
import random

import fheregex as F

LIMITS = [8, 16, 17, 64]            # run on the device
LENGTHS = LIMITS + [32, 33, 63]     # run on the CPU
WIDEST = {8, 16, 32, 63, 64}        # the lengths with a chunk of 16 tests; within LIMITS: 8, 16, 64

# 80 bytes of period 8 with one deviant: Q Q Q Q Q' Q Q Q Q Q, where Q' is Q with its last byte
# 0x80 replaced by 0x00 (position 39; the two differ in the high nibble alone, the last of a
# needle's 2 m tests).  Bytes >= 0x80 and letters of both cases in every period, one 0x00.
Q = b"aB\xe9c\xffdE\x80"
DEVIANT = 39
TEXT = Q * 4 + Q[:7] + b"\x00" + Q * 5
assert len(TEXT) == 80 and TEXT.count(0) == 1 and TEXT[DEVIANT] == 0


def needle(m, text=TEXT):
    """the window at the last start that fits"""
    return text[len(text) - m:]


def absent(s):
    """s with its last byte's high nibble changed: every occurrence of s is a near miss of it"""
    return s[:-1] + bytes([s[-1] ^ 0x40])


def starts_of(text, masks):
    from test_private_needle_gpu import py_starts
    return py_starts(text, masks)


def cases(m, text=TEXT):
    """(name, masks) of the needles of length m: the window at the last start as it is, in the
    other case under ignore_case, with its first, middle and last byte a wildcard (the near miss
    then matches), and the absent variant"""
    s = needle(m, text)
    wild = bytearray(s)
    wild[0] = wild[m // 2] = wild[m - 1] = ord("?")
    assert b"?" not in text and s.swapcase() != s
    return [("plain", F.needle_masks(s)), ("ignore-case", F.needle_masks(s.swapcase(), ignore_case=True)),
            ("wildcard", F.needle_masks(bytes(wild), any_char="?")), ("absent", F.needle_masks(absent(s)))]


def ranges(n, m):
    """[lo, hi): the whole text, ranges that end just before, on and after the last start that
    fits, that start on and after it, one past the text's end and an empty one"""
    last = n - m
    return [(0, n), (0, last), (0, last + 1), (last, last + 1), (last, n + 2), (last + 1, n), (max(last - 1, 0), last + 2),
            (last, last)]


def check_plain(evaluator, m, text=TEXT):
    """the plaintext evaluator against py_starts for every needle of cases(m) over every range"""
    n = len(text)
    for name, masks in cases(m, text):
        want = starts_of(text, masks)
        assert (want == []) == (name == "absent"), (m, name, want)
        assert name == "absent" or n - m in want  # the last start that fits
        for lo, hi in ranges(n, m):
            bits = [int(p in want) for p in range(lo, hi)]
            assert evaluator(text, masks, lo, hi) == (bits, int(any(bits))), (evaluator.__name__, m, name, lo, hi)
    return starts_of(text, cases(m, text)[0][1])


def check_every_test_counts(evaluator, m, text=TEXT):
    """each of the 2 m tables emptied in turn: the needle no longer occurs, so every selector
    (term) index of range(2 m) is read, at its own content nibble"""
    masks = F.needle_masks(needle(m, text))
    last = len(text) - m
    assert evaluator(text, masks, last, last + 1) == ([1], 1)
    for t in range(2 * m):
        one = [list(lh) for lh in masks]
        one[t // 2][t % 2] = 0xFFFF ^ one[t // 2][t % 2]  # every nibble value but the needle's
        assert evaluator(text, [tuple(lh) for lh in one], last, last + 1) == ([0], 0), (evaluator.__name__, m, t)


def known_starts(m):
    """where needle(m) occurs in TEXT and where its near miss (all but the last byte) does, from
    the period: a window free of the deviant recurs every 8 bytes on either side of it, one that
    ends on it is a near miss, and one that holds it further in occurs once"""
    last = len(TEXT) - m
    if last <= DEVIANT:  # m >= 41: the needle holds the deviant
        return [last], []
    occ = [p for p in range(last % 8, last + 1, 8) if not p <= DEVIANT < p + m]
    return occ, [DEVIANT - m + 1] if (DEVIANT - m + 1) % 8 == last % 8 else []


# the device's texts: slices of TEXT short enough for the oracle (a find costs 2 m rotations a start)
DEVICE_TEXT = {
    8: TEXT[24:48],    # Q Q' Q: the needle at 0 and 16 (the last start), its near miss at 8; 17 starts
    16: TEXT[24:56],   # Q Q' Q Q: the needle at 16 (the last start), its near miss at 0; 17 starts
    17: TEXT[39:64],   # 0x00 Q Q Q: the needle at 8 (the last start) of 9
    64: TEXT[14:80],   # 66 bytes: three starts, the needle (it holds the 0x00) at 2
}
TEXT_65 = TEXT[15:80]  # two starts: level 1 of a find is 2 * 128 = 256 rotations
# a scan's texts.  Windows of 64 bytes recur only where the deviant is out of sight, so TEXT goes on
# for five more periods: the 17 windows from 40 on are 8 distinct ones, the last start's at 40, 48, 56
SCAN_TEXT = TEXT + Q * 5
# and 130 seeded bytes: 67 distinct windows of 64 bytes, padded to 128, the compacted text's
# positions up to 8,191
RANDOM_TEXT = random.Random(20261021).randbytes(130)


def tree_levels(n):
    """jobs per level of a balanced threshold tree over n literals, fan-in 16"""
    out = []
    while n > 1:
        n = (n + 15) // 16
        out.append(n)
    return out


def chunk_lens(m):
    from selector_cases import balanced_chunks
    chunks = balanced_chunks(2 * m)
    assert [a for a, _ in chunks] == [sum(ln for _, ln in chunks[:i]) for i in range(len(chunks))]
    assert sum(ln for _, ln in chunks) == 2 * m and all(1 <= ln <= 16 for _, ln in chunks)
    return [ln for _, ln in chunks]


def level_jobs(m, fit, starts, clear):
    """jobs per level of a find over `fit` starts that fit, from balanced_chunks(2 m) and or_tree
    alone.  Encrypted content: 2 m selector jobs a start, a sign gate per chunk, the AND of the
    chunks; clear content: the chunks' sums are no jobs, a sign gate reads each.  Then the OR over
    the starts, unless every start is an output."""
    from test_find_clear import or_tree
    if fit == 0:
        return []
    chunks = len(chunk_lens(m))
    levels = ([] if clear else [2 * m * fit]) + [chunks * fit] + [fit * c for c in tree_levels(chunks)]
    if not starts:
        levels += tree_levels(fit)
        assert sum(tree_levels(fit)) == or_tree(fit)
    assert sum(tree_levels(chunks)) == or_tree(chunks)
    return levels


def check_levels(S, m, fit, starts, clear):
    """the schedule S has the derived jobs per level; every sign gate over a chunk has
    offset = 1 - 2 len (clear: over its one sum; encrypted: over its len tests); the chunk ANDs
    and the ORs have theirs; returns the level-1 jobs"""
    want = level_jobs(m, fit, starts, clear)
    got = [S.level_off[i + 1] - S.level_off[i] for i in range(len(S.level_off) - 1)]
    assert got == want, (m, fit, starts, clear, got, want)
    assert len(S.jobs) == sum(want)
    if fit == 0:
        return []
    lens = chunk_lens(m)
    at = 0 if clear else 1
    gates = S.jobs[S.level_off[at]:S.level_off[at + 1]]
    for i, j in enumerate(gates):
        ln = lens[i % len(lens)]
        assert j.kind == F.JOB_SIGN and j.n_out == 1 and j.offset == 1 - 2 * ln, (m, i, j.offset, ln)
        assert j.n_in == (1 if clear else ln) and all(j.in_w[q] == 1 for q in range(j.n_in))
    assert (max(lens) == 16) == (m in WIDEST) == (min(j.offset for j in gates) == -31)
    if m in LIMITS:
        assert (max(lens) == 16) == (m in (8, 16, 64))
    if len(lens) > 1:  # the AND of a start's chunks
        for j in S.jobs[S.level_off[at + 1]:S.level_off[at + 2]]:
            assert (j.kind, j.n_in, j.offset) == (F.JOB_SIGN, len(lens), 1 - 2 * len(lens))
    for j in S.jobs[S.level_off[at + 1 + len(tree_levels(len(lens)))]:]:  # the OR tree
        assert j.kind == F.JOB_SIGN and j.offset == -1 and 2 <= j.n_in <= 16
    return S.jobs[:S.level_off[1]]
