"""Byte-table needles on the device: the byte variant of the extract-sum kernel word for word
against the numpy restatement of tests/byte_needle_cases.py, fr_find_clear* and fr_scan_clear* with
a byte-table needle end to end and, output by output, against Oracle.run_schedule; the plan cache
keyed by the needle's form, lanes, the extract-sum's noise and the refusals.

Contexts and oracles are tests/test_gate_programs.py's, the end-to-end contexts (with a packing
key) tests/test_private_needle_gpu.py's."""
import ctypes as C

import numpy as np
import pytest

import byte_needle_cases as bc
import fheregex as F
import selector_cases as sc
import test_gate_programs as tg
import test_private_needle_gpu as pn

pytestmark = pytest.mark.gpu

U = np.uint64
PIDS = list(bc.POINTS)
_NEEDLE = {}


def tpg(c):
    return c.params.N // 256


def kernel_needle(key_blob, monkeypatch, pid):
    """an m = TPG + 3 needle of random tables on the point's default context (two selectors):
    (context, needle, its selectors on the host)"""
    if pid not in _NEEDLE:
        c = tg.device_ctx(key_blob, monkeypatch, pid, {})
        rng = np.random.default_rng(177)
        tables = [int.from_bytes(rng.bytes(32), "little") for _ in range(tpg(c) + 3)]
        blob = c.encrypt_needle_bytes(tables, seed=178)
        _NEEDLE[pid] = c, c.upload_needle(blob), c.expand_needle_bytes(blob)
    return _NEEDLE[pid]


def assert_words(c, nd, sel, content, sums, what):
    got = c.dev_select_sum(nd, content, sums)
    assert got.shape == (len(sums), c.lwe_len)
    for i, terms in enumerate(sums):
        want = bc.extract_sum_bytes(sel, content, terms)
        assert np.array_equal(got[i], want), (what, i, terms, np.flatnonzero(got[i] != want)[:8])


# ------------------------------------------------------------------ the kernel, word for word
@pytest.mark.parametrize("pid", PIDS)
def test_kernel_words(key_blob, monkeypatch, pid):
    c, nd, sel = kernel_needle(key_blob, monkeypatch, pid)
    k, N, T = c.params.k, c.params.N, tpg(c)
    m = T + 3
    assert len(nd) == m and nd.form == F.NEEDLE_BYTES and sel.shape == (2, k + 1, N) and sel[:, :k].any()
    content = bytes([0x00, 0xFF, 0x41, 0x7F, 0x80, 0x0F, 0xF0, 0x39])
    # one term at table slot 0 and slot TPG - 1 with bytes 0x00 and 0xFF: j = 0 and j = N - 1 among them
    assert_words(c, nd, sel, content, [[(0, 0, 0)], [(0, 1, 0)], [(T - 1, 0, 0)], [(T - 1, 1, 0)]], "one term")
    neg = lambda x: -int(x) % 2 ** 64  # noqa: E731
    first = c.dev_select_sum(nd, content, [[(0, 0, 0)]])[0]  # j = 0: every word but the first is negated
    assert first[0] == sel[0, 0, 0] and int(first[1]) == neg(sel[0, 0, N - 1]) and first[k * N] == sel[0, k, 0]
    assert int(first[N - 1]) == neg(sel[0, 0, 1])
    last = c.dev_select_sum(nd, content, [[(T - 1, 1, 0)]])[0]  # j = N - 1: none is
    assert last[0] == sel[0, 0, N - 1] and last[N - 1] == sel[0, 0, 0] and last[k * N] == sel[0, k, N - 1]
    if k == 2:
        assert int(first[N + 1]) == neg(sel[0, 1, N - 1]) and last[2 * N - 1] == sel[0, 1, 0]
    # every table at every content byte: coefficients that are no multiple of N/16, both selectors
    assert_words(c, nd, sel, content, [[(i, pos, 0)] for i in range(m) for pos in range(len(content))], "every slot")
    rng = np.random.default_rng(179)
    sixteen = [[(int(i), int(p), 0) for i, p in zip(rng.integers(0, m, 16), rng.integers(0, 8, 16))]]
    assert_words(c, nd, sel, content, sixteen, "sixteen terms")
    span = [[(T - 1, 1, 0), (T, 0, 0)], [(0, 2, 0), (m - 1, 7, 0), (T, 7, 0)]]  # terms in both selectors
    assert_words(c, nd, sel, content, span, "a sum across two selectors")
    assert_words(c, nd, sel, content, [[(2, 1, 0), (2, 3, 0)], [(2, 3, 0), (2, 3, 0)]], "a table twice")
    for count in (1, 2, 65):  # a block per sum, 1 to 16 terms each
        sums = [[(int(rng.integers(0, m)), int(rng.integers(0, 8)), 0) for _ in range(1 + (i * 7 + count) % 16)]
                for i in range(count)]
        assert_words(c, nd, sel, content, sums, "launch of %d" % count)


def test_a_nibble_needle_still_runs_the_nibble_kernel(key_blob, monkeypatch):
    """the variant follows the bound needle: a nibble needle after a byte needle on one context"""
    from test_find_clear import extract_sum
    c, nd, sel = kernel_needle(key_blob, monkeypatch, "k1n2048")
    blob = c.encrypt_needle([(1 << 3, 0xFFFF), (0x00F0, 1 << 4)], seed=180)
    nib, nsel = c.upload_needle(blob), c.expand_needle(blob)
    assert nib.form == F.NEEDLE_NIBBLES
    content, terms = b"\x13\x4e", [(0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 1, 1)]
    assert np.array_equal(c.dev_select_sum(nib, content, [terms])[0], extract_sum(nsel, content, terms))
    assert_words(c, nd, sel, content, [[(1, 0, 0), (2, 1, 0)]], "and back")
    nib.close()


def test_hook_refusals(key_blob, monkeypatch):
    c, nd, sel = kernel_needle(key_blob, monkeypatch, "k1n2048")
    m = len(nd)
    before = c.device_timers(), c.arena_stats()
    for text, sums in ((b"ab", [[(0, 0, 1)]]), (b"ab", [[(0, 0, 2)]]), (b"ab", [[(0, 0, 0), (1, 1, -1)]]),  # third field
                       (b"ab", [[(m, 0, 0)]]), (b"ab", [[(0, 0, 0)], [(63, 1, 0)]]), (b"ab", [[(-1, 0, 0)]]),  # i >= m
                       (b"ab", [[(0, 2, 0)]]), (b"", [[(0, 0, 0)]]), (b"ab", [[]]), (b"ab", [[(0, 0, 0)] * 17])):
        with pytest.raises(F.FheRegexError):
            c.dev_select_sum(nd, text, sums)
    assert (c.device_timers(), c.arena_stats()) == before
    assert c.dev_select_sum(nd, b"ab", [[(m - 1, 1, 0)]]).any()  # the last of each bound is accepted


# ------------------------------------------------------------------ end to end
def lengths(pid):
    T = bc.POINTS[pid][1] // 256
    return [1, T, T + 1, 16, 17] + ([64] if pid == "k1n2048" else [])


def check_finds(c, ck, sk, nd, text, want):
    """the four searches and both reply forms against the starts `want`"""
    bits = [int(p in want) for p in range(len(text))]
    handles = c.handle_count()
    for fn in (c.find_clear, c.scan_clear):
        out, _ = fn(text, nd)
        assert ck.decrypt(out) == int(bool(want)), fn.__name__
        c.release(out)
    hs = c.find_clear_starts(text, nd)
    assert [ck.decrypt(h) for h in hs] == bits
    for h in hs:
        c.release(h)
    for compact in (False, True):
        got, ref = sk.scan_clear_starts(text, nd, compact), sk.find_clear_starts(text, nd, compact)
        assert got == ref, (compact, [i for i in range(min(len(got), len(ref))) if got[i] != ref[i]][:8])
        assert ck.decrypt_starts(got) == want
    assert c.handle_count() == handles


@pytest.mark.parametrize("pid,m", [(pid, m) for pid in PIDS for m in lengths(pid)])
def test_finds_end_to_end(key_blob, pid, m):
    """literals, [0-9], [^x], . and \\w at every length at which the lowering or the packing of
    tables changes shape; one needle that matches and one that does not"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    if True:
        text = bc.text_for(m)
        assert len(text) == (80 if m == 64 else 40)
        pat = bc.pattern(m)
        tables = F.needle_tables(pat)
        want = [p for p, v in enumerate(bc.py_find(text, tables, 0, len(text))) if v]
        assert 0 in want and F.plain_find_clear_bytes(text, tables)[1] == 1
        nd = sk.upload_needle(ck.encrypt_needle_classes(pat, seed=300 + m))
        assert len(nd) == m and nd.form == F.NEEDLE_BYTES
        S = F.schedule_find_clear_bytes(len(text), m, starts=True)
        hs, st = c.find_clear_starts(text, nd, stats=True)
        assert st.pbs == st.blind_rotations == len(S.jobs) and st.levels == len(S.level_off) - 1
        for h in hs:
            c.release(h)
        check_finds(c, ck, sk, nd, text, want)
        nd.close()
        # the last position's class emptied of the byte it met: no start matches
        none = tables[:-1] + [tables[-1] & ~sum(1 << b for b in {text[p + m - 1] for p in want})]
        nd = sk.upload_needle(c.encrypt_needle_bytes(none, seed=400 + m))  # (an empty table is a table)
        assert bc.py_find(text, none, 0, len(text)) == [0] * len(text)
        check_finds(c, ck, sk, nd, text, [])
        nd.close()


@pytest.mark.parametrize("pid", PIDS)
def test_product_classes_answer_as_the_nibble_needle(key_blob, pid):
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    text = bc.TEXT
    for s, ic, wc in (("Id ?0", False, "?"), ("id 40", True, None), ("7", False, None)):
        masks = F.needle_masks(s, ic, wc)
        tables = [sum(1 << b for b in range(256) if (lo >> (b & 15)) & 1 and (hi >> (b >> 4)) & 1) for lo, hi in masks]
        assert all(bc.product_masks(t) == mk for t, mk in zip(tables, masks))
        nib = sk.upload_needle(c.encrypt_needle(masks, seed=501))
        byt = sk.upload_needle(c.encrypt_needle_bytes(tables, seed=502))
        assert (nib.form, byt.form, len(nib), len(byt)) == (F.NEEDLE_NIBBLES, F.NEEDLE_BYTES, len(s), len(s))
        want = pn.py_starts(text, masks)
        assert want and want == [p for p, v in enumerate(bc.py_find(text, tables, 0, len(text))) if v]
        for compact in (False, True):
            a, b = sk.find_clear_starts(text, nib, compact), sk.find_clear_starts(text, byt, compact)
            assert ck.decrypt_starts(a) == ck.decrypt_starts(b) == want
            assert ck.decrypt_starts(sk.scan_clear_starts(text, byt, compact)) == want
        oa, ob = sk.find_clear(text, nib), sk.find_clear(text, byt)
        assert ck.decrypt(oa) == ck.decrypt(ob) == 1
        c.release(oa), c.release(ob)
        nib.close(), byt.close()


# ------------------------------------------------------------------ pinned to the oracle
def byte_values(S, sel, text, m):
    """{gate: LWE} of a byte find's extract-sums: start by start, chunk by chunk of the m tests,
    term t = (table t, position p + t, 0); the gates are the level-1 jobs' single inputs, in order"""
    lvl1 = S.jobs[:S.level_off[1]] if len(S.level_off) > 1 else []
    gates = [j.in_ref[0] for j in lvl1]
    sums = [[(t, p + t, 0) for t in range(first, first + ln)]
            for p in range(len(text) - m + 1) for first, ln in sc.balanced_chunks(m)]
    assert len(sums) == len(gates) == len(set(gates))
    return {g: bc.extract_sum_bytes(sel, text, terms) for g, terms in zip(gates, sums)}


def oracle_words(O, sel, m, text, starts):
    S = F.schedule_find_clear_bytes(len(text), m, starts=starts)
    O.run_schedule(S, None, values=byte_values(S, sel, text, m))
    return np.stack([O._output(*p) for p in S.parts])


@pytest.mark.parametrize("m", [3, 17])
@pytest.mark.parametrize("pid", PIDS)
def test_find_clear_words(request, key_blob, pid, m):
    """every output of fr_find_clear_starts and fr_find_clear word for word against
    Oracle.run_schedule on the byte schedule, its extract-sums from extract_sum_bytes over
    fr_expand_needle_bytes' selectors (m = 17: two sums of 9 and 8 terms and an AND a start)"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    text = bc.TEXT
    blob = ck.encrypt_needle_classes(bc.pattern(m), seed=600 + m)
    sel = c.expand_needle_bytes(blob)
    nd = sk.upload_needle(blob)
    try:
        out, _ = c.find_clear(text, nd)
        hs = c.find_clear_starts(text, nd)
        got = pn.output_words(c, [out] + hs)
        assert ck.decrypt(out) == 1 and ck.decrypt(hs[0]) == 1
        for h in [out] + hs:
            c.release(h)
        want = np.concatenate([oracle_words(O, sel, m, text, False), oracle_words(O, sel, m, text, True)])
        assert got.shape == want.shape == (1 + len(text), c.lwe_len)
        bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], want[i])]  # (-1: fr_find_clear's)
        assert not bad, (pid, m, bad)
    finally:
        nd.close()


# ------------------------------------------------------------------ plan cache, lanes, release
def test_cache_is_keyed_by_the_form(key_blob):
    c, ck, sk, _, _ = pn.e2e(key_blob, "k1n2048")
    t1, t2 = bc.TEXT, bc.TEXT[::-1]
    s = "Id 40"
    nib = sk.upload_needle(ck.encrypt_needle(s, seed=701))
    byt = sk.upload_needle(ck.encrypt_needle_classes(r"Id [0-9]\w", seed=702))
    byt2 = sk.upload_needle(ck.encrypt_needle_classes(r"\w[^x]...", seed=703))
    starts = lambda hs: [p for p, h in enumerate(hs) if ck.decrypt(h)]  # noqa: E731
    want = lambda t, pat: [p for p, v in enumerate(bc.py_find(t, F.needle_tables(pat), 0, len(t))) if v]  # noqa: E731
    c.set_plan_cache(0), c.set_plan_cache(8)
    try:
        a, sa = c.find_clear_starts(t1, nib, stats=True)
        b, sb = c.find_clear_starts(t1, byt, stats=True)  # the same (m, n), the other form: a plan of its own
        assert (sa.plan_cached, sb.plan_cached) == (0, 0) and c.plan_cache_stats()["entries"] == 2
        assert sa.pbs == sb.pbs == 36  # m = 5: one rotation per start either way
        assert starts(a) == [p for p in range(40) if t1.startswith(b"Id 40", p)] == [0, 20]
        assert starts(b) == want(t1, r"Id [0-9]\w") == [0, 20]
        d, sd = c.find_clear_starts(t1, byt2, stats=True)  # a second byte needle of the same m: a hit
        e, se = c.find_clear_starts(t2, byt, stats=True)  # a second text of the same length: a hit
        f, sf = c.find_clear_starts(t1, nib, stats=True)  # and the nibble plan is still its own
        assert (sd.plan_cached, se.plan_cached, sf.plan_cached) == (1, 1, 1)
        assert c.plan_cache_stats()["entries"] == 2
        assert starts(d) == want(t1, r"\w[^x]...") != [] and starts(e) == want(t2, r"Id [0-9]\w") and starts(f) == [0, 20]
        for h in a + b + d + e + f:
            c.release(h)
        # two asynchronous lanes reproduce the serial words
        serial = []
        for nd in (byt, byt2):
            hs = c.find_clear_starts(t1, nd)
            serial.append(pn.output_words(c, hs))
            for h in hs:
                c.release(h)
        c.set_lanes(2)
        c.set_async(True)
        for rep in range(2):  # (the first round compiles each lane's plan copy)
            outs = [c.find_clear_starts(t1, nd) for nd in (byt, byt2, byt2, byt)]
            for hs, ref in zip(outs, (serial[0], serial[1], serial[1], serial[0])):
                assert np.array_equal(pn.output_words(c, hs), ref), rep
                for h in hs:
                    c.release(h)
        # the needle may go right after an asynchronous find: the release waits for every lane
        last = sk.upload_needle(ck.encrypt_needle_classes(r"Id [0-9]\w", seed=702))
        hs = c.find_clear_starts(t1, last)
        last.close()
        assert np.array_equal(pn.output_words(c, hs), serial[0])
        for h in hs:
            c.release(h)
    finally:
        c.set_async(False)
        c.set_lanes(1)
        nib.close(), byt.close(), byt2.close()


# ------------------------------------------------------------------ the extract-sum's noise
@pytest.mark.parametrize("pid", PIDS)
def test_sum_noise_is_sixteen_fresh_coefficients(request, key_blob, pid):
    """a sum of 16 terms carries 16 independent fresh GLWE coefficients' errors, a
    gaussian of deviation 4 sigma 2^64; every sum of the m = 16 find stays under 8 deviations,
    32 sigma 2^64 (2^17.4 at (1, 2048)) -- derived from sigma, not from a run"""
    c, ck, sk, _, _ = pn.e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    text, m = bc.TEXT, 16
    tables = F.needle_tables(bc.pattern(m))
    blob = c.encrypt_needle_bytes(tables, seed=801)
    nd = c.upload_needle(blob)
    sums = [[(t, p + t, 0) for t in range(m)] for p in range(len(text) - m + 1)]
    lwes = c.dev_select_sum(nd, text, sums)
    nd.close()
    counts = [sum((tables[t] >> text[p + t]) & 1 for t in range(m)) for p in range(len(sums))]
    assert counts[0] == 16 and min(counts) < 16
    err = (O.phase(lwes) - (np.array(counts, dtype=U) << U(59))).view(np.int64)
    bound = 8 * 4 * c.params.glwe_sigma * 2.0 ** 64
    worst = float(np.abs(err).max())
    print("%s: largest extract-sum error 2^%.1f, bound 2^%.1f" % (pid, np.log2(max(worst, 1)), np.log2(bound)))
    assert bound < 2 ** 20 and worst < bound


# ------------------------------------------------------------------ refusals
def test_refusals(key_blob, monkeypatch):
    """an error code each, and nothing planned or launched"""
    c1, ck1, sk1, hs1, _ = pn.e2e(key_blob, "k1n2048")
    c2, ck2, sk2, _, _ = pn.e2e(key_blob, "k2n1024")
    n1 = sk1.upload_needle(ck1.encrypt_needle_classes("a[b-c]c", seed=901))
    n2 = sk2.upload_needle(ck2.encrypt_needle_classes("a[b-c]c", seed=902))
    state = lambda c: (c.plan_cache_stats(), c.arena_stats(), c.device_timers())  # noqa: E731
    out = (C.c_uint32 * 64)()
    L = F.lib()

    def clear_rcs(c, text, nd):
        n = C.c_size_t()
        return (L.fr_find_clear(c.h, text, len(text), nd.h, 0, len(text), out, None),
                L.fr_find_clear_starts(c.h, text, len(text), nd.h, 0, len(text), out, None),
                L.fr_scan_clear(c.h, text, len(text), nd.h, 0, len(text), out, None),
                L.fr_scan_clear_starts(c.h, text, len(text), nd.h, 0, len(text), 1, None, 0, C.byref(n), None))

    # fr_find and fr_find_starts need rotations of the needle's tables
    c1.set_profiling(1)
    try:
        before = state(c1)
        content = np.ascontiguousarray(hs1, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
        assert L.fr_find(c1.h, content, len(hs1), n1.h, 0, len(hs1), out, None) == F.ERR_INVALID
        assert "clear content only" in L.fr_last_error().decode()
        assert L.fr_find_starts(c1.h, content, len(hs1), n1.h, 0, len(hs1), out, None) == F.ERR_INVALID
        with pytest.raises(F.FheRegexError):
            sk1.find(hs1, n1)
        with pytest.raises(F.FheRegexError):
            sk1.find_starts(hs1, n1)
        assert state(c1) == before
    finally:
        c1.set_profiling(0)
    # an RNS context: no needle of either form, no search
    rns = tg.device_ctx(key_blob, monkeypatch, "rns", {})
    blob = ck1.encrypt_needle_classes("abc", seed=903)
    h = C.c_void_p()
    before = state(rns)
    assert L.fr_upload_needle(rns.h, blob, len(blob), C.byref(h)) == F.ERR_INVALID
    assert "FFT ring only" in L.fr_last_error().decode()
    assert clear_rcs(rns, b"xxabcxx", n1) == (F.ERR_INVALID,) * 4
    assert state(rns) == before
    # the other (k, N), and the same (k, N) on another context
    other = tg.device_ctx(key_blob, monkeypatch, "k1n2048", {})
    for c, nd in ((c1, n2), (c2, n1), (other, n1)):
        before = state(c)
        assert clear_rcs(c, b"xxabcxx", nd) == (F.ERR_INVALID,) * 4
        assert state(c) == before
    assert L.fr_upload_needle(c2.h, blob, len(blob), C.byref(h)) == F.ERR_INVALID  # a blob of the other (k, N)
    # and the needle still answers where it belongs
    o = sk1.find_clear(b"xxabcxx", n1)
    assert ck1.decrypt(o) == 1
    c1.release(o)
    n1.close(), n2.close()
