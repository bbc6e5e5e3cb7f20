"""Private search over clear content on the device: the extract-sum kernel (k_select_sum) word for
word against the numpy restatement of tests/test_find_clear.py, fr_find_clear /
fr_find_clear_starts end to end, the plan cache and the per-call binding of the content bytes,
lanes, ownership of the sum slots, the packed replies and the refusals.  Whole finds are also
compared output by output with Oracle.run_schedule, its extract-sums seeded from the numpy
restatement over the needle's expanded selectors: every level above the sums, word for word.

Contexts and oracles are tests/test_gate_programs.py's, the end-to-end contexts (with a packing
key) and the content tests/test_private_needle_gpu.py's, so that every find over clear content
stands next to fr_find on an encryption of the same text."""
import ctypes as C

import numpy as np
import pytest

import fheregex as F
import selector_cases as sc
import test_gate_programs as tg
import test_private_needle_gpu as pn
from test_find_clear import extract_sum

pytestmark = pytest.mark.gpu

U = np.uint64
PIDS = ["k1n2048", "k2n1024"]
# No 16 bytes hold 0x00, 0x0F, 0xF0 and 0xFF and still every nibble value in both halves (0x00 and
# 0xF0 share their low nibble), so the kernel reads two 16-byte contents: every value once in
# each half, with 0x0F and 0xF0; and one with 0x00 and 0xFF, j = 0 and j = 15 N/16 in both halves
PERM = bytes(v | ((15 - v) << 4) for v in range(16))
EDGE = bytes([0x00, 0x0F, 0xF0, 0xFF, 0x12, 0x23, 0x34, 0x45, 0x56, 0x67, 0x78, 0x89, 0x9A, 0xAB, 0xBC, 0xCD])
_BIG = {}


def big_needle(key_blob, monkeypatch, pid):
    """an m = 64 needle of random masks on the point's default context: (context, needle, its
    128 selectors on the host)"""
    if pid not in _BIG:
        c = tg.device_ctx(key_blob, monkeypatch, pid, {})
        rng = np.random.default_rng(77)
        masks = [(int(a), int(b)) for a, b in rng.integers(0, 1 << 16, (64, 2))]
        blob = c.encrypt_needle(masks, seed=78)
        _BIG[pid] = c, c.upload_needle(blob), c.expand_needle(blob)
    return _BIG[pid]


def assert_words(c, nd, sel, content, sums, what):
    got = c.dev_select_sum(nd, content, sums)
    assert got.shape == (len(sums), c.lwe_len)
    for i, terms in enumerate(sums):
        want = extract_sum(sel, content, terms)
        assert np.array_equal(got[i], want), (what, i, terms, np.flatnonzero(got[i] != want)[:8])


# ------------------------------------------------------------------ the kernel, word for word
@pytest.mark.parametrize("pid", PIDS)
def test_kernel_words(key_blob, monkeypatch, pid):
    c, nd, sel = big_needle(key_blob, monkeypatch, pid)
    k, N = c.params.k, c.params.N
    assert sel.shape == (128, k + 1, N) and sel[:, :k].any()
    rng = np.random.default_rng(79)
    for content in (PERM, EDGE):
        # one term: every position and half (every nibble value, j = 0 and j = 15 N/16 among them)
        assert_words(c, nd, sel, content, [[(int(rng.integers(0, 128)), pos, h)] for pos in range(16) for h in (0, 1)],
                     "one term")
    # at k = 2 both mask polynomials and the body differ from term to term: checked by all of the above
    one = c.dev_select_sum(nd, EDGE, [[(5, 0, 0)]])[0]  # j = 0: word 0 alone is not negated
    neg = lambda x: -int(x) % 2 ** 64  # noqa: E731
    assert one[0] == sel[5, 0, 0] and int(one[1]) == neg(sel[5, 0, N - 1]) and one[k * N] == sel[5, k, 0]
    if k == 2:
        assert one[N] == sel[5, 1, 0] and int(one[N + 1]) == neg(sel[5, 1, N - 1])
    two = [[(3, 2, 0), (4, 2, 1)], [(0, 0, 0), (127, 15, 1)]]
    assert_words(c, nd, sel, EDGE, two, "two terms")
    sixteen = [[(int(q), int(p), int(h)) for q, p, h in zip(rng.integers(0, 128, 16), rng.integers(0, 16, 16),
                                                             rng.integers(0, 2, 16))] for _ in range(3)]
    assert_words(c, nd, sel, PERM, sixteen, "sixteen terms")
    # the last selector of the longest needle, the last position
    assert_words(c, nd, sel, EDGE, [[(127, 15, 0)], [(127, 15, 1), (126, 14, 0)]], "selector 127, position len - 1")
    # one selector at two positions of one sum, and twice at the same one
    assert_words(c, nd, sel, PERM, [[(9, 1, 0), (9, 7, 0)], [(9, 3, 1), (9, 3, 1)]], "a selector twice")
    # launches of 1, 3 and 257 sums (a block per sum: a tail past 256), 1 to 16 terms each
    for count in (1, 3, 257):
        sums = [[(int(rng.integers(0, 128)), int(rng.integers(0, 16)), int(rng.integers(0, 2)))
                 for _ in range(1 + (i * 7 + count) % 16)] for i in range(count)]
        assert_words(c, nd, sel, EDGE if count % 2 else PERM, sums, "launch of %d" % count)


def test_hook_refusals(key_blob, monkeypatch):
    c, nd, sel = big_needle(key_blob, monkeypatch, "k1n2048")
    small = c.upload_needle(c.encrypt_needle(F.needle_masks("ab"), seed=80))
    before = c.device_timers(), c.arena_stats()
    for needle, text, sums in ((nd, PERM, [[]]), (nd, PERM, [[(0, 0, 0)] * 17]), (small, PERM, [[(4, 0, 0)]]),
                               (nd, PERM, [[(0, 16, 0)]]), (nd, b"", [[(0, 0, 0)]]), (nd, PERM, [[(0, 0, 2)]]),
                               (nd, PERM, [[(0, 0, 0)], [(-1, 0, 0)]]), (nd, PERM, [[(0, -1, 0)]])):
        with pytest.raises(F.FheRegexError):
            c.dev_select_sum(needle, text, sums)
    assert (c.device_timers(), c.arena_stats()) == before
    assert c.dev_select_sum(small, PERM, [[(3, 15, 1)]]).any()  # the last of each bound is accepted
    small.close()


# ------------------------------------------------------------------ end to end
CONTENT = pn.CONTENT
HIGH = b"x\xe9\x80y\xe9\x80\xe9\x00\xff\xe9\x80zz\xe9\x80\xe9"  # 16 bytes, some >= 0x80, a 0x00
_ENC = {}


def encrypted(c, pid, text: bytes):
    """content handles of any bytes (encrypt_str takes ASCII only): four 2-bit blocks a byte, low first"""
    if (pid, text) not in _ENC:
        blocks = c.encrypt_blocks([(b >> (2 * i)) & 3 for b in text for i in range(4)], seed=12)
        _ENC[pid, text] = c.upload_radix(blocks)
    return _ENC[pid, text]


def check_outputs(request, c, ck, pid, handles, want_bits):
    """decryption, and every output's phase error under the oracle's big key below 2^53"""
    O = tg.oracle(request, pid)
    words = np.stack([c.download_radix(h)[0] for h in handles])
    assert [ck.decrypt(h) for h in handles] == want_bits
    err = (O.phase(words) - (np.array(want_bits, dtype=U) << U(59))).view(np.int64)
    worst = int(np.abs(err).max())
    print("%s: largest phase error 2^%.1f" % (pid, np.log2(max(worst, 1))))
    assert worst < 2 ** 53, np.log2(worst)


CASES = [(CONTENT.encode(), s.encode(), ic, wc) for s, ic, wc in pn.NEEDLES] + [(HIGH, b"\xe9\x80", False, None)]


@pytest.mark.parametrize("case", CASES, ids=[(s.decode("latin-1") + ("-i" if ic else "")).replace("\xe9\x80", "high")
                                            for _, s, ic, _ in CASES])
@pytest.mark.parametrize("pid", PIDS)
def test_find_clear_and_find_clear_starts(request, key_blob, pid, case):
    c, ck, sk, hs, _ = pn.e2e(key_blob, pid)
    text, s, ignore_case, any_char = case
    masks = F.needle_masks(s, ignore_case, any_char)
    want = pn.py_starts(text.decode("latin-1"), masks) if text == CONTENT.encode() else [
        p for p in range(len(text)) if text.startswith(s, p)]
    assert F.plain_find_clear(text, masks) == ([int(p in want) for p in range(len(text))], int(bool(want)))
    bits = [int(p in want) for p in range(len(text))]
    nd = sk.upload_needle(c.encrypt_needle(masks, seed=21))
    enc = hs if text == CONTENT.encode() else encrypted(c, pid, text)
    c.set_profiling(1)
    try:
        for starts in (True, False):
            S = F.schedule_find_clear(len(text), len(s), starts=starts)
            t0 = c.device_timers()
            if starts:
                outs, st = c.find_clear_starts(text, nd, stats=True)
                want_bits = bits
            else:
                out, st = c.find_clear(text, nd)
                outs, want_bits = [out], [int(bool(want))]
            assert c.device_timers()["br_gates"] - t0["br_gates"] == len(S.jobs)  # (synchronises)
            assert st.pbs == st.blind_rotations == len(S.jobs) and st.levels == len(S.level_off) - 1
            check_outputs(request, c, ck, pid, outs, want_bits)
            ref = c.find_starts(enc, nd) if starts else [c.find(enc, nd)[0]]
            assert [ck.decrypt(h) for h in ref] == want_bits  # fr_find* on an encryption of the same text
            for h in outs + ref:
                c.release(h)
    finally:
        c.set_profiling(0)
        nd.close()


def device_find_clear_words(c, nd, text):
    """block 0 of fr_find_clear's output, then of every output of fr_find_clear_starts"""
    out, _ = c.find_clear(text, nd)
    starts = c.find_clear_starts(text, nd)
    try:
        return pn.output_words(c, [out] + starts)
    finally:
        for h in [out] + starts:
            c.release(h)


def oracle_find_clear_words(O, sel, m, text):
    return np.concatenate([sc.oracle_find(O, sel, m, text=text), sc.oracle_find(O, sel, m, text=text, starts=True)])


@pytest.mark.parametrize("s", pn.WORD_NEEDLES)
@pytest.mark.parametrize("pid", PIDS)
def test_find_clear_words(request, key_blob, pid, s):
    """Whole finds over clear content word for word: every output of fr_find_clear and
    fr_find_clear_starts against Oracle.run_schedule on the same schedule, whose extract-sums are
    extract_sum over fr_expand_needle's selectors (m = 9: two sums and a two-level AND a start)."""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    text = CONTENT.encode()
    blob = ck.encrypt_needle(s, seed=21)
    sel = c.expand_needle(blob)
    nd = sk.upload_needle(blob)
    try:
        got, want = device_find_clear_words(c, nd, text), oracle_find_clear_words(O, sel, len(s), text)
        assert got.shape == want.shape == (1 + len(text), c.lwe_len)
        bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], want[i])]  # (-1: fr_find_clear's)
        assert not bad, (pid, s, bad)
    finally:
        nd.close()


def test_find_clear_words_on_two_lanes(request, key_blob):
    """the same comparison with two lanes, asynchronous: the serial run's words and the oracle's"""
    c, ck, sk, _, _ = pn.e2e(key_blob, "k1n2048")
    O = tg.oracle(request, "k1n2048")
    text = CONTENT.encode()
    blob = ck.encrypt_needle("abc", seed=21)
    want = oracle_find_clear_words(O, c.expand_needle(blob), 3, text)
    nd = sk.upload_needle(blob)
    try:
        serial = device_find_clear_words(c, nd, text)
        assert np.array_equal(serial, want)
        c.set_lanes(2)
        c.set_async(True)
        for rep in range(2):  # (the first round compiles each lane's plan copy)
            assert np.array_equal(device_find_clear_words(c, nd, text), serial), rep
    finally:
        c.set_lanes(1)
        nd.close()


@pytest.mark.parametrize("pid", PIDS)
def test_shapes(request, key_blob, pid):
    """m = 9 (the AND is a tree over two sums), m > n_chars, partial ranges, hi past the end"""
    c, ck, sk, hs, _ = pn.e2e(key_blob, pid)
    text = CONTENT.encode()
    nine = sk.upload_needle(ck.encrypt_needle(CONTENT[2:11], seed=23))
    outs, st = c.find_clear_starts(text, nine, stats=True)
    assert st.levels == 2 and st.pbs == 3 * 8
    check_outputs(request, c, ck, pid, outs, [int(p == 2) for p in range(16)])
    out, st = c.find_clear(text, nine)
    assert st.levels == 3 and ck.decrypt(out) == 1
    for h in outs + [out]:
        c.release(h)
    nine.close()
    nd = sk.upload_needle(ck.encrypt_needle("abcde", seed=24))
    out, st = c.find_clear(b"abcd", nd)  # m > n_chars: the constant, nothing launched
    assert ck.decrypt(out) == 0 and st.pbs == 0
    starts = c.find_clear_starts(b"abcd", nd)
    assert [ck.decrypt(h) for h in starts] == [0, 0, 0, 0]
    for h in starts + [out]:
        c.release(h)
    nd.close()
    nd = sk.upload_needle(ck.encrypt_needle("ab", seed=25))  # at 2, 14; "Ab" at 7 is none
    for lo, hi, any_ in ((0, 16, 1), (3, 14, 0), (3, 15, 1), (14, 16, 1), (15, 16, 0), (5, 5, 0)):
        out, st = c.find_clear(text, nd, lo, hi)
        assert ck.decrypt(out) == any_, (lo, hi)
        c.release(out)
    hs_ = c.find_clear_starts(text, nd, 12, 19)  # past the end: starts that cannot fit are trivial 0s
    assert [ck.decrypt(h) for h in hs_] == [0, 0, 1, 0, 0, 0, 0]
    a, st_a = c.find_clear(text, nd, 0, 16)
    b, st_b = c.find_clear(text, nd, 0, 2 ** 63)  # the range cut at the content: the same plan
    assert st_b.plan_cached == 1 and (ck.decrypt(a), ck.decrypt(b)) == (1, 1)
    for h in hs_ + [a, b]:
        c.release(h)
    nd.close()


# ------------------------------------------------------------------ plan cache and binding
def test_cache_is_keyed_by_shape_and_the_bytes_travel_per_call(key_blob):
    c, ck, sk, hs, _ = pn.e2e(key_blob, "k1n2048")
    a = sk.upload_needle(ck.encrypt_needle("abc", seed=31))
    b = sk.upload_needle(ck.encrypt_needle("zab", seed=32))
    t1, t2 = CONTENT.encode(), b"zabzabxxxxxxxabc"  # abc at 2 / at 13; zab at none / at 0, 3
    o1 = c.find_clear_starts(t1, a)
    stats = c.plan_cache_stats()
    o2, st2 = c.find_clear_starts(t2, a, stats=True)  # a second text of the same length: a hit, its own answer
    assert st2.plan_cached == 1 and c.plan_cache_stats()["hits"] == stats["hits"] + 1
    o3, st3 = c.find_clear_starts(t2, b, stats=True)  # a second needle of the same m: a hit
    assert st3.plan_cached == 1 and c.plan_cache_stats()["entries"] == stats["entries"]
    o4 = c.find_clear_starts(t1, b)
    o5 = c.find_clear_starts(t1, a)  # and back: the plan holds nothing of t2 or b
    got = [[p for p, h in enumerate(o) if ck.decrypt(h)] for o in (o1, o2, o3, o4, o5)]
    assert got == [[2], [13], [0, 3], [], [2]]
    # fr_find_starts with the same (m, n) does not share the entry, either way round
    misses = c.plan_cache_stats()["misses"]
    c.set_plan_cache(0), c.set_plan_cache(8)
    f = c.find_starts(hs, a)
    o6, st6 = c.find_clear_starts(t1, a, stats=True)
    f2, stf = c.find_starts(hs, a, stats=True)
    assert st6.plan_cached == 0 and stf.plan_cached == 1 and c.plan_cache_stats()["misses"] == misses + 2
    assert c.plan_cache_stats()["entries"] == 2
    assert [p for p, h in enumerate(o6) if ck.decrypt(h)] == [p for p, h in enumerate(f2) if ck.decrypt(h)] == [2]
    for h in o1 + o2 + o3 + o4 + o5 + o6 + f + f2:
        c.release(h)
    a.close(), b.close()


def test_lanes_two_texts_back_to_back(key_blob):
    """with two lanes, asynchronous finds over two different texts queued back to back give each
    its own answer, word for word the serial run's"""
    c, ck, sk, hs, _ = pn.e2e(key_blob, "k1n2048")
    t1, t2 = CONTENT.encode(), b"zabzabxxxxxxxabc"
    blob = ck.encrypt_needle("abc", seed=41)
    nd = sk.upload_needle(blob)
    serial = []
    for t in (t1, t2):
        out = c.find_clear(t, nd)[0]
        serial.append(c.download_radix(out))
        c.release(out)
    c.set_lanes(2)
    c.set_async(True)
    try:
        for rep in range(2):  # (the first round compiles each lane's plan copy)
            outs = [c.find_clear(t, nd)[0] for t in (t1, t2, t2, t1)]
            words = [c.download_radix(h) for h in outs]
            for w, want in zip(words, (serial[0], serial[1], serial[1], serial[0])):
                assert np.array_equal(w, want), rep
            assert [ck.decrypt(h) for h in outs] == [1, 1, 1, 1]
            for h in outs:
                c.release(h)
        starts = [c.find_clear_starts(t, nd) for t in (t1, t2)]
        assert [[p for p, h in enumerate(o) if ck.decrypt(h)] for o in starts] == [[2], [13]]
        for h in starts[0] + starts[1]:
            c.release(h)
    finally:
        c.set_lanes(1)
        nd.close()


def test_ownership(key_blob):
    """the sum slots are the plan's: outputs released and the cache emptied, arena and handle
    counts are where they were; the needle may be closed right after asynchronous finds"""
    c, ck, sk, hs, _ = pn.e2e(key_blob, "k1n2048")
    blob = ck.encrypt_needle("abc", seed=51)
    c.set_plan_cache(0), c.set_plan_cache(8)
    arena, handles = c.arena_stats(), c.handle_count()
    c.set_lanes(2)
    try:
        nd = sk.upload_needle(blob)
        outs = [c.find_clear(CONTENT.encode(), nd)[0] for _ in range(4)]
        outs += c.find_clear_starts(CONTENT.encode(), nd)
        nd.close()  # asynchronous finds may still be queued: the release waits for every lane
        assert [ck.decrypt(h) for h in outs] == [1] * 4 + [int(p == 2) for p in range(16)]
        assert c.plan_cache_stats()["slots"] > 0
        for h in outs:
            c.release(h)
        c.set_plan_cache(0)
        after = c.arena_stats()
        assert after["slots"] - after["free_slots"] == arena["slots"] - arena["free_slots"]
        assert c.handle_count() == handles
        # the uncached path (no plan kept: staged descriptors on lane 0) owns and returns its slots too
        nd = sk.upload_needle(blob)
        out, st = c.find_clear(CONTENT.encode(), nd)
        assert st.plan_cached == 0 and ck.decrypt(out) == 1 and c.plan_cache_stats()["entries"] == 0
        c.release(out)
        nd.close()
        after = c.arena_stats()
        assert after["slots"] - after["free_slots"] == arena["slots"] - arena["free_slots"]
    finally:
        c.set_plan_cache(8)
        c.set_lanes(1)


# ------------------------------------------------------------------ replies
@pytest.mark.parametrize("pid", PIDS)
def test_packed_replies(key_blob, pid):
    c, ck, sk, hs, _ = pn.e2e(key_blob, pid)
    for s, ic, wc in pn.NEEDLES[:3]:
        nd = sk.upload_needle(ck.encrypt_needle(s, ic, wc, seed=61))
        want = pn.py_starts(CONTENT, F.needle_masks(s, ic, wc))
        handles = c.handle_count()
        for compact in (False, True):
            assert ck.decrypt_starts(sk.find_clear_starts(CONTENT, nd, compact=compact)) == want, (s, compact)
        out = sk.find_clear(CONTENT, nd)
        assert ck.decrypt(out) == int(bool(want))
        c.release(out)
        assert c.handle_count() == handles
        nd.close()


# ------------------------------------------------------------------ refusals
def find_clear_rc(c, text, needle_h):
    out = (C.c_uint32 * max(len(text), 1))()
    return (F.lib().fr_find_clear(c.h, text, len(text), needle_h, 0, len(text), out, None),
            F.lib().fr_find_clear_starts(c.h, text, len(text), needle_h, 0, len(text), out, None))


def test_refusals(key_blob, monkeypatch):
    """an error code each, and nothing planned or launched"""
    c1, ck1, sk1, _, _ = pn.e2e(key_blob, "k1n2048")
    c2, ck2, sk2, _, _ = pn.e2e(key_blob, "k2n1024")
    n1 = sk1.upload_needle(ck1.encrypt_needle("abc", seed=71))
    n2 = sk2.upload_needle(ck2.encrypt_needle("abc", seed=72))
    state = lambda c: (c.plan_cache_stats(), c.arena_stats(), c.device_timers())  # noqa: E731
    both = (F.ERR_INVALID, F.ERR_INVALID)
    rns = tg.device_ctx(key_blob, monkeypatch, "rns", {})
    rns.set_profiling(1)
    try:
        before = state(rns)
        assert find_clear_rc(rns, b"abcd", n1.h) == both
        assert "FFT ring only" in F.lib().fr_last_error().decode()
        assert state(rns) == before
    finally:
        rns.set_profiling(0)
    other = tg.device_ctx(key_blob, monkeypatch, "k1n2048", {})  # the same (k, N), another context
    for c, needle in ((c1, n2), (c2, n1), (other, n1)):
        c.set_profiling(1)
        try:
            before = state(c)
            assert find_clear_rc(c, b"xxabcxx", needle.h) == both
            out = (C.c_uint32 * 8)()
            assert F.lib().fr_find_clear(c.h, None, 4, needle.h, 0, 4, out, None) == F.ERR_INVALID
            assert state(c) == before
        finally:
            c.set_profiling(0)
    before = state(c1)
    out = (C.c_uint32 * 8)()
    assert F.lib().fr_find_clear(c1.h, None, 4, n1.h, 0, 4, out, None) == F.ERR_INVALID
    assert F.lib().fr_find_clear(c1.h, b"abcd", 4, n1.h, 3, 2, out, None) == F.ERR_INVALID
    assert F.lib().fr_find_clear_starts(c1.h, b"abcd", 4, n1.h, 0, 2 ** 63, out, None) == F.ERR_INVALID
    assert state(c1) == before
    n1.close(), n2.close()
