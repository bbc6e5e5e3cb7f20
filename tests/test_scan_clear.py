"""Scan of a long clear text, host side (include/fheregex.h): the window classes
(fr_window_classes), the lowering over the compacted text (fr_schedule_scan_clear), its plaintext
evaluation (fr_plain_scan_clear) and the mapped packing keyswitch's host restatement
(fr_pack_lwes_mapped).  No device: the kernel and the scans are tests/test_scan_clear_gpu.py."""
import ctypes as C
import random

import numpy as np
import pytest

import fheregex as F
import needle_limits as nl
from selector_cases import balanced_chunks
from test_find_clear import or_tree, py_find
from test_packed_results import POINTS, PSEED, host

BUCKET = 64  # lower.h SCAN_BUCKET


# ------------------------------------------------------------------ window classes
def py_classes(text: bytes, m, lo, hi):
    """the restatement: classes in order of first appearance over the starts of [lo, min(hi, n))"""
    seen, cls = {}, []
    for p in range(lo, min(hi, len(text))):
        if p + m > len(text):
            cls.append(-1)
            continue
        w = text[p:p + m]
        cls.append(seen.setdefault(w, len(seen)))
    return cls, len(seen), -(-len(seen) // BUCKET) * BUCKET, b"".join(seen)


def test_window_classes_against_python():
    """200 seeded texts over all byte values (half of them over two values, so that windows
    recur): lengths 0..80, m 1..9, random ranges, hi past the end, lo = hi, m > n"""
    rng = random.Random(20251021)
    repeats = 0
    for case in range(200):
        n, m = rng.randint(0, 80), rng.randint(1, 9)
        alphabet = bytes(range(256)) if case % 2 else b"\x00\xff"
        text = bytes(rng.choice(alphabet) for _ in range(n))
        lo = rng.randint(0, n)
        hi = rng.choice([lo, rng.randint(lo, n), n, n + rng.randint(1, 5), 2 ** 40])
        got, want = F.window_classes(text, m, lo, hi), py_classes(text, m, lo, hi)
        assert got == want, (case, text, m, lo, hi)
        fit = [c for c in got[0] if c >= 0]
        repeats += len(fit) > got[1]
        # every start's window is its class's, byte for byte
        for j, c in enumerate(got[0]):
            assert c < 0 or got[3][c * m:(c + 1) * m] == text[lo + j:lo + j + m]
    assert repeats > 30  # classes were shared in many of the cases
    assert F.window_classes(b"abc", 5) == ([-1, -1, -1], 0, 0, b"")  # m > n
    assert F.window_classes(b"", 1) == ([], 0, 0, b"")


def test_window_classes_planted():
    assert F.window_classes(b"a" * 40, 3) == ([0] * 38 + [-1, -1], 1, 64, b"aaa")  # all equal: D = 1
    text = bytes(range(256))
    cls, D, Dpad, win = F.window_classes(text, 1)  # all distinct, D a multiple of the bucket
    assert (cls, D, Dpad, win) == (list(range(256)), 256, 256, text)
    assert F.window_classes(text[:65], 1)[1:3] == (65, 128)
    # windows that differ in the last byte only, and in a 0x00 only (no C-string comparison)
    assert F.window_classes(b"abcabd", 3, 0, 4) == ([0, 1, 2, 3], 4, 64, b"abcbcacababd")
    assert F.window_classes(b"a\x00ba\x00c", 3)[0] == [0, 1, 2, 3, -1, -1]
    assert F.window_classes(b"a\x00\x00a\x00\x01a\x00\x00", 3)[0] == [0, 1, 2, 3, 4, 5, 0, -1, -1]
    assert F.window_classes(b"\x00\x00\x00\x00", 2) == ([0, 0, 0, -1], 1, 64, b"\x00\x00")
    n, d, dp = C.c_size_t(), C.c_uint64(), C.c_uint64()
    fn = F.lib().fr_window_classes
    for bad in ((b"abc", 3, 0, 0, 3), (b"abc", 3, 65, 0, 3), (b"abc", 3, 2, 3, 2)):  # m = 0, m = 65, lo > hi
        assert fn(*bad, None, 0, C.byref(n), C.byref(d), C.byref(dp), None, 0) == F.ERR_INVALID
    cls = (C.c_int32 * 2)()
    assert fn(b"abc", 3, 1, 0, 3, cls, 2, C.byref(n), C.byref(d), C.byref(dp), None, 0) == F.ERR_INVALID  # cls_cap


# ------------------------------------------------------------------ lowering
@pytest.mark.parametrize("Dpad,m", [(64, 1), (64, 3), (64, 8), (128, 3), (320, 2), (64, 9), (64, 64)])
@pytest.mark.parametrize("starts", [False, True])
def test_schedule(Dpad, m, starts):
    """2 m <= 16: Dpad sign gates over one extract-sum each, then the balanced OR tree over Dpad
    (64 + 4 + 1 at Dpad = 64); beyond, a sign gate per balanced chunk of the 2 m tests and their
    AND per window first"""
    S = F.schedule_scan_clear(Dpad, m, starts=starts)
    assert all(j.kind == F.JOB_SIGN for j in S.jobs)
    chunks = [2 * m] if 2 * m <= 16 else [ln for _, ln in balanced_chunks(2 * m)]
    lvl1 = S.jobs[:S.level_off[1]]
    assert len(lvl1) == len(chunks) * Dpad
    made = {j.out_gate[0] for j in S.jobs}
    for i, j in enumerate(lvl1):
        assert (j.n_in, j.n_out, j.in_w[0], j.offset) == (1, 1, 1, 1 - 2 * chunks[i % len(chunks)])
        assert j.in_ref[0] >= 0 and j.in_ref[0] not in made
    assert len({j.in_ref[0] for j in lvl1}) == len(lvl1)
    and_jobs = Dpad * or_tree(len(chunks))  # the AND over a window's chunks (fan-in 16)
    and_levels = 1
    n = len(chunks)
    while n > 1:
        n = (n + 15) // 16
        and_levels += 1
    or_levels = 0
    n = Dpad
    while n > 1:
        n = (n + 15) // 16
        or_levels += 1
    if starts:
        assert len(S.jobs) == len(lvl1) + and_jobs and len(S.level_off) - 1 == and_levels
        assert len(S.parts) == Dpad and all(p[0] >= 0 and p[1:] == (1, 0) for p in S.parts)
        assert len({p[0] for p in S.parts}) == Dpad
    else:
        assert len(S.jobs) == len(lvl1) + and_jobs + or_tree(Dpad)
        assert len(S.level_off) - 1 == and_levels + or_levels
        assert len(S.parts) == 1 and S.parts[0][1:] == (1, 0)


def test_rotation_totals():
    assert len(F.schedule_scan_clear(64, 3).jobs) == 64 + 4 + 1
    assert len(F.schedule_scan_clear(64, 8).jobs) == 64 + 4 + 1
    assert len(F.schedule_scan_clear(64, 9).jobs) == 2 * 64 + 64 + 4 + 1
    assert len(F.schedule_scan_clear(64, 64).jobs) == 8 * 64 + 64 + 4 + 1
    assert len(F.schedule_scan_clear(1664, 3, starts=True).jobs) == 1664
    assert F.schedule_scan_clear(0, 3).parts == [(-1, 0, 0)] and F.schedule_scan_clear(0, 3, starts=True).parts == []


def job_bytes(S):
    return [C.string_at(C.addressof(j), C.sizeof(j)) for j in S.jobs]


@pytest.mark.parametrize("n", [1, 16, 64, 100])
@pytest.mark.parametrize("starts", [False, True])
def test_stride_one_is_find_clear(n, starts):
    """m = 1 is stride 1: the generalised lowering emits fr_schedule_find_clear's program, every
    job byte for byte (a job's in_ref names its extract-sum's gate, so the sums sit at the same
    program gates too), the levels and the outputs"""
    a, b = F.schedule_scan_clear(n, 1, starts=starts), F.schedule_find_clear(n, 1, starts=starts)
    assert job_bytes(a) == job_bytes(b) and len(a.jobs) > 0
    assert (a.level_off, a.parts, a.n_gates) == (b.level_off, b.parts, b.n_gates)


def test_stride_m_reads_the_compacted_text():
    """the extract-sums of windows of m bytes read bytes d m .. d m + m - 1: evaluated on a text
    of distinct windows, output d says whether window d is the needle"""
    m, text = 3, b"abcabdxbcab\x00"
    cls, D, Dpad, win = F.window_classes(text, m)
    assert D == 8 and win[:6] == b"abcbca"  # bca and cab recur
    for needle in (b"abc", b"ab\x00", b"bca", b"zzz"):
        starts, any_ = F.plain_scan_clear(text, F.needle_masks(needle))
        assert starts == [int(text[p:p + m] == needle) for p in range(len(text))]
        assert any_ == int(needle in text)


def test_schedule_bounds():
    nj, nl, ns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    outs = (C.c_int32 * 3)()
    fn = F.lib().fr_schedule_scan_clear
    for m in (0, 65):
        assert fn(64, m, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
    assert fn(2 ** 24, 2, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
    assert fn(64, 3, 2, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
    assert fn(64, 3, 1, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 63, C.byref(ns)) == F.ERR_INVALID


# ------------------------------------------------------------------ plain evaluation
def test_plain_scan_clear_against_python():
    """200 seeded (content, needle, range) cases in tests/test_find_clear.py's style: every start
    (rebuilt through the classes) and the OR, against the Python search, bytes.find and
    fr_plain_find_clear"""
    rng = random.Random(20251022)
    hits = shared = 0
    for case in range(200):
        n, m = rng.randint(1, 40), min(rng.randint(1, 12), rng.randint(1, 12))
        alphabet = bytes(range(256)) if case % 4 == 0 else b"\x00aA\xe9\xc9\xff"[:rng.randint(2, 6)]
        content = bytes(rng.choice(alphabet) for _ in range(n))
        if rng.random() < 0.7 and m <= n:
            at = rng.randint(0, n - m)
            needle = bytearray(content[at:at + m])
        else:
            needle = bytearray(rng.choice(alphabet) for _ in range(m))
        ignore_case = rng.random() < 0.4
        if ignore_case:
            needle = bytearray(bytes(needle).swapcase() if rng.random() < 0.5 else needle)
        wild = rng.random() < 0.4
        if wild:
            for i in range(m):
                if rng.random() < 0.3:
                    needle[i] = ord("?")
        lo = rng.randint(0, n // 2)
        hi = rng.randint((lo + n) // 2, n + 2)
        masks = F.needle_masks(bytes(needle), ignore_case, "?" if wild else None)
        starts, any_ = F.plain_scan_clear(content, masks, lo, hi)
        want = py_find(content, masks, lo, hi)
        assert starts == want, (case, content, bytes(needle), ignore_case, wild, lo, hi)
        assert any_ == int(any(want)), case
        assert (starts, any_) == F.plain_find_clear(content, masks, lo, hi), case
        if not ignore_case and not wild:
            assert starts == [int(content.find(bytes(needle), p, p + m) == p) for p in range(lo, hi)], case
        cls, D, _, _ = F.window_classes(content, m, lo, hi)
        shared += D < sum(c >= 0 for c in cls)
        hits += any_
    assert 40 < hits < 190 and shared > 40  # both answers occur often, and so do shared windows


def test_three_plain_evaluators_on_one_text():
    """fr_plain_find, fr_plain_find_clear and fr_plain_scan_clear evaluate through one body: all
    three against the Python search on one 12-byte text whose 3-byte window recurs, a 3-character
    needle -- the whole range, a range cut at the text's end, empty ranges -- and a needle longer
    than the text (the random cases above reach these only by chance, and never all three calls)"""
    text = b"abcxabcabcyz"
    assert F.window_classes(text, 3)[1] == 8  # ten windows fit; abc is three of them
    evaluators = (F.plain_find, F.plain_find_clear, F.plain_scan_clear)
    for needle in (b"abc", b"abcxabcabcyzq"):
        masks = F.needle_masks(needle)
        for lo, hi in ((0, 12), (0, None), (3, 17), (11, 14), (12, 15), (4, 4), (0, 0), (12, 12)):
            want = py_find(text, masks, lo, 12 if hi is None else hi)
            for f in evaluators:
                assert f(text, masks, lo, hi) == (want, int(any(want))), (f.__name__, needle, lo, hi)
    assert py_find(text, F.needle_masks(b"abc"), 0, 12) == [1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------ the needle-length limits
@pytest.mark.parametrize("m", nl.LENGTHS)
def test_plain_scan_clear_at_the_length_limits(m):
    """fr_plain_scan_clear against py_starts on needle_limits.TEXT and on its continuation, whose
    windows recur at every length: the window at d m of the compacted text is window d's"""
    assert nl.check_plain(F.plain_scan_clear, m) == nl.known_starts(m)[0]
    nl.check_every_test_counts(F.plain_scan_clear, m)
    text = nl.SCAN_TEXT
    occ = nl.check_plain(F.plain_scan_clear, m, text)
    cls, D, Dpad, win = F.window_classes(text, m)
    fit = len(text) - m + 1
    assert len(occ) >= 3 and D < fit and Dpad == 64
    assert all(win[c * m:(c + 1) * m] == text[p:p + m] for p, c in enumerate(cls[:fit]))


def test_plain_scan_clear_past_64_windows_of_64_bytes():
    """130 seeded bytes, m = 64: 67 distinct windows, padded to 128, so the plan's text is 8,192
    bytes and window d's terms read d 64 .. d 64 + 63; the needle is the last window (class 66),
    the first, one in the middle, and absent"""
    text, m = nl.RANDOM_TEXT, 64
    cls, D, Dpad, win = F.window_classes(text, m)
    assert (D, Dpad, len(win)) == (67, 128, 67 * 64) and cls[:67] == list(range(67))
    for at in (66, 0, 33):
        masks = F.needle_masks(text[at:at + m])
        assert nl.starts_of(text, masks) == [at]
        for lo, hi in nl.ranges(len(text), m):
            bits = [int(p == at) for p in range(lo, hi)]
            assert F.plain_scan_clear(text, masks, lo, hi) == (bits, int(any(bits))), (at, lo, hi)
    nl.check_every_test_counts(F.plain_scan_clear, m, text)
    assert F.plain_scan_clear(text, F.needle_masks(nl.absent(text[66:])))[1] == 0


@pytest.mark.parametrize("m", nl.LENGTHS)
@pytest.mark.parametrize("Dpad", [64, 128])
@pytest.mark.parametrize("starts", [False, True])
def test_schedule_at_the_length_limits(Dpad, m, starts):
    """fr_schedule_scan_clear is find_clear's shape over Dpad starts that all fit"""
    S = F.schedule_scan_clear(Dpad, m, starts=starts)
    lvl1 = nl.check_levels(S, m, Dpad, starts, clear=True)
    made = {j.out_gate[0] for j in S.jobs}
    sums = [j.in_ref[0] for j in lvl1]
    assert all(g >= 0 and g not in made for g in sums) and len(set(sums)) == len(sums) == Dpad * len(nl.chunk_lens(m))
    assert len(S.parts) == (Dpad if starts else 1) and all(p[0] >= 0 and p[1:] == (1, 0) for p in S.parts)


# ------------------------------------------------------------------ the mapped pack on the host
@pytest.fixture(scope="module")
def keyed(key_blob):
    ctx = host(POINTS[0], key_blob)
    ctx.gen_packing_key(PSEED)
    return ctx


def test_pack_host_mapped(keyed):
    rng = np.random.default_rng(5)
    R = 5
    lwes = keyed.encrypt_blocks(rng.integers(0, 2, R).astype(np.uint8), seed=78).reshape(R, -1)
    w, off = [1, -1, 1, 0, 1], [0, 2, 0, 2, 0]  # a negated row and a constant among them
    # the identity map over n rows is pack_host
    assert np.array_equal(keyed.pack_lwes_mapped(lwes, range(R), w, off), keyed.pack_lwes(lwes, w, off))
    # a map with repeats is pack_host over the rows expanded start by start
    map_ = [0, 1, 1, 4, 2, 0, 3, 3, 4, 0, 2]
    want = keyed.pack_lwes(lwes[map_], [w[r] for r in map_], [off[r] for r in map_])
    assert np.array_equal(keyed.pack_lwes_mapped(lwes, map_, w, off), want)
    # a -1 entry contributes nothing: the constant 0 (weight 0, offset 0) in the expanded list
    gaps = [0, -1, 1, 4, -1, 2, 0, 3, -1, -1]
    want = keyed.pack_lwes(lwes[[max(r, 0) for r in gaps]], [w[r] if r >= 0 else 0 for r in gaps],
                           [off[r] if r >= 0 else 0 for r in gaps])
    assert np.array_equal(keyed.pack_lwes_mapped(lwes, gaps, w, off), want)
    # the last start, N - 1, wraps every coefficient but one
    N = keyed.params.N
    last = [-1] * (N - 1) + [0]
    one = keyed.pack_lwes(lwes[:1])
    got = keyed.pack_lwes_mapped(lwes[:1], last)
    for c in range(2):
        a, b = one[c * N:(c + 1) * N], got[c * N:(c + 1) * N]
        assert b[N - 1] == a[0] and np.array_equal(b[:N - 1], (-a[1:].astype(np.int64)).astype(np.uint64))


def test_pack_host_mapped_refusals(keyed):
    lwes = np.zeros((3, keyed.lwe_len), dtype=np.uint64)
    N = keyed.params.N
    for rows, map_ in ((3, [0, 1, 3]),        # an entry >= R
                       (3, [0, 1, 1]),        # a row no start reads
                       (3, [0, 1, -1]),       # ... a -1 does not read it either
                       (3, [0, 1]),           # R > n
                       (1, [0] * (N + 1))):   # n > N
        with pytest.raises(F.FheRegexError):
            keyed.pack_lwes_mapped(lwes[:rows], map_)
    out = np.zeros(2 * N, dtype=np.uint64)
    mp = (C.c_int32 * 1)(0)
    assert F.lib().fr_pack_lwes_mapped(keyed.h, F._p(lwes), None, None, 0, mp, 1, F._p(out)) == F.ERR_INVALID  # R < 1
    bare = host(POINTS[0])
    assert F.lib().fr_pack_lwes_mapped(bare.h, F._p(lwes), None, None, 1, mp, 1, F._p(out)) == F.ERR_INVALID  # no key


# ------------------------------------------------------------------ header, symbols, refusals
NEW = ["fr_scan_clear", "fr_scan_clear_starts", "fr_scan_classes", "fr_window_classes", "fr_schedule_scan_clear",
       "fr_plain_scan_clear", "fr_dev_pack_mapped", "fr_pack_lwes_mapped"]


def test_header_and_symbols():
    syms = F.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(F.lib(), name), name
        assert name in F._SIGS, name


def test_refusals_on_a_host_only_context(key_blob):
    c = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_FFT))
    c.load_client_key(key_blob)
    needle = C.create_string_buffer(256)  # never read: a host-only context has no needle to give
    nd = C.cast(needle, C.c_void_p)
    out = (C.c_uint32 * 4)()
    n = C.c_size_t()
    buf = C.create_string_buffer(64)
    lib = F.lib()
    assert lib.fr_scan_clear(c.h, b"abcd", 4, nd, 0, 4, out, None) == F.ERR_NO_DEVICE
    assert lib.fr_scan_clear(c.h, None, 4, nd, 0, 4, out, None) == F.ERR_INVALID
    assert lib.fr_scan_clear(c.h, b"abcd", 4, nd, 3, 2, out, None) == F.ERR_INVALID
    assert lib.fr_scan_clear(c.h, b"abcd", 4, None, 0, 4, out, None) == F.ERR_INVALID
    assert lib.fr_scan_clear_starts(c.h, b"abcd", 4, nd, 0, 4, 0, buf, 64, C.byref(n), None) == F.ERR_NO_DEVICE
    assert lib.fr_scan_clear_starts(c.h, b"abcd", 4, nd, 0, 4, 2, buf, 64, C.byref(n), None) == F.ERR_INVALID
    assert lib.fr_scan_clear_starts(c.h, b"abcd", 4, nd, 0, 4, 0, buf, 64, None, None) == F.ERR_INVALID
    assert lib.fr_scan_clear_starts(c.h, b"abcd", 4, nd, 0, 2 ** 24 + 1, 0, buf, 64, C.byref(n), None) == F.ERR_INVALID
    hs = (C.c_uint32 * 1)(0)
    mp = (C.c_int32 * 1)(0)
    assert lib.fr_dev_pack_mapped(c.h, hs, 1, mp, 1, 0, buf, 64, C.byref(n)) == F.ERR_NO_DEVICE
    assert c.scan_classes() == (0, 0)
