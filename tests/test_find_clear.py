"""Private search over clear content, host side (include/fheregex.h): the lowering of
fr_find_clear / fr_find_clear_starts (fr_schedule_find_clear), its plaintext evaluation
(fr_plain_find_clear), and the sample extract the first level rests on, restated in numpy and
checked against the selectors of an encrypted needle.  No device: the kernel and the finds are
tests/test_find_clear_gpu.py."""
import ctypes as C
import random
import time

import numpy as np
import pytest

import fheregex as F
import needle_limits as nl
import oracle_ffi as of

U = np.uint64
K = bytes((29 * i + 3) & 0xFF for i in range(32))  # a fixed 256-bit generator key
TABLES = [1 << 5, (1 << 4) | (1 << 6), 0xFFFF, 0]  # one bit, two bits, all ones, none
POINTS = {"k1n2048": (1, 2048), "k2n1024": (2, 1024)}


# ------------------------------------------------------------------ the formula, restated
def extract_sum(sel, content, terms):
    """out[c N + t] = sum over (q, pos, h) of (t <= j ? A_{q,c}[j - t] : -A_{q,c}[N + j - t]),
    out[k N] = sum of B_q[j], with j = ((content[pos] >> 4 h) & 15) N / 16; sel is
    [selector][k + 1][N] u64 (mask polynomials, then the body).  Wrapping u64."""
    k, N = sel.shape[1] - 1, sel.shape[2]
    out = np.zeros(k * N + 1, dtype=U)
    t = np.arange(N)
    with np.errstate(over="ignore"):
        for q, pos, h in terms:
            j = ((content[pos] >> (4 * h)) & 15) * (N // 16)
            for c in range(k):
                a = sel[q, c][(j - t) % N]
                out[c * N:(c + 1) * N] += np.where(t <= j, a, U(0) - a)
            out[k * N] += sel[q, k, j]
    return out


def direct_poly(N, table):
    """V(lut) of test_poly<N>(t, direct = true, lut) for the 0/1 table `table`"""
    mm = (np.arange(N) + N // 32) // (N // 16)
    bit = lambda s: ((table >> s) & 1) << 59  # noqa: E731
    return np.array([bit(int(s)) if s < 16 else -bit(0) % 2 ** 64 for s in mm], dtype=U)


# ------------------------------------------------------------------ schedule
def or_tree(n):
    """jobs of a balanced threshold tree over n literals, fan-in 16"""
    jobs = 0
    while n > 1:
        n = (n + 15) // 16
        jobs += n
    return jobs


@pytest.mark.parametrize("n_chars,m", [(16, 1), (16, 3), (16, 8), (16, 9), (5, 5), (4, 5)])
@pytest.mark.parametrize("starts", [False, True])
def test_schedule(n_chars, m, starts):
    S = F.schedule_find_clear(n_chars, m, starts=starts)
    fit = max(n_chars - m + 1, 0)
    assert not any(j.kind == F.JOB_ACC for j in S.jobs)  # no selector job anywhere
    assert all(j.kind == F.JOB_SIGN for j in S.jobs)
    if fit == 0:  # (4, 5): no job, the constant 0
        assert S.jobs == [] and S.level_off == [0]
        assert S.parts == ([(-1, 0, 0)] * n_chars if starts else [(-1, 0, 0)])
        return
    made = {j.out_gate[0] for j in S.jobs}
    lvl1 = S.jobs[:S.level_off[1]]
    # level 1: one sign job per chunk per fitting start, each over one extract-sum (a program
    # gate that no job makes), weight 1, the AND's offset over the chunk's terms
    chunks = [2 * m] if 2 * m <= 16 else [m, m]
    assert len(lvl1) == len(chunks) * fit
    for i, j in enumerate(lvl1):
        assert (j.n_in, j.n_out, j.in_w[0], j.offset) == (1, 1, 1, 1 - 2 * chunks[i % len(chunks)])
        assert j.in_ref[0] >= 0 and j.in_ref[0] not in made
    assert len({j.in_ref[0] for j in lvl1}) == len(lvl1)  # a sum of its own each
    if len(chunks) == 1:
        and_levels, tops = 1, [j.out_gate[0] for j in lvl1]
    else:  # (16, 9): two levels per start
        lvl2 = S.jobs[S.level_off[1]:S.level_off[2]]
        assert len(lvl2) == fit and all(j.n_in == 2 and j.offset == -3 for j in lvl2)
        for p, j in enumerate(lvl2):
            assert [j.in_ref[0], j.in_ref[1]] == [lvl1[2 * p].out_gate[0], lvl1[2 * p + 1].out_gate[0]]
        and_levels, tops = 2, [j.out_gate[0] for j in lvl2]
    if starts:
        assert len(S.level_off) - 1 == and_levels  # 2 m <= 16: exactly 1 level
        assert S.parts[:fit] == [(g, 1, 0) for g in tops]
        assert S.parts[fit:] == [(-1, 0, 0)] * (n_chars - fit)  # a start that cannot fit: the constant 0
    else:
        or_jobs = S.jobs[S.level_off[and_levels]:]
        assert len(or_jobs) == or_tree(fit)
        if fit > 1:
            assert len(or_jobs) == 1 and or_jobs[0].n_in == fit and or_jobs[0].offset == -1
            assert sorted(or_jobs[0].in_ref[:fit]) == sorted(tops)
        assert len(S.parts) == 1 and S.parts[0][1:] == (1, 0)


def test_rotation_totals_at_256_by_3():
    """one rotation per fitting start, then the OR tree: 254 and 254 + 16 + 1 = 271, against
    fr_find's 2 m more per start"""
    n, m = 256, 3
    fit = n - m + 1
    assert (fit, fit + or_tree(fit)) == (254, 271)
    S = F.schedule_find_clear(n, m, starts=True)
    assert (len(S.jobs), len(S.level_off) - 1) == (fit, 1)
    S = F.schedule_find_clear(n, m)
    assert (len(S.jobs), len(S.level_off) - 1) == (fit + or_tree(fit), 3)
    assert len(F.schedule_find(n, m).jobs) == 2 * m * fit + fit + or_tree(fit) == 1795


def test_schedule_bounds():
    """fr_schedule_find's, one for one"""
    nj = C.c_size_t()
    outs = (C.c_int32 * 3)()
    fn = F.lib().fr_schedule_find_clear
    for m in (0, 65):
        assert fn(16, m, 0, 16, 0, None, 0, C.byref(nj), None, 0, C.byref(nj), outs, 1, C.byref(nj)) == F.ERR_INVALID
    assert len(F.schedule_find_clear(80, 64).jobs) > 0
    far = F.schedule_find_clear(16, 3, 2, 16)
    nl, ns = C.c_size_t(), C.c_size_t()
    F._check(fn(16, 3, 2, 2 ** 63, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)))
    assert (nj.value, nl.value, ns.value) == (len(far.jobs), len(far.level_off) - 1, 1)
    assert fn(16, 3, 0, 2 ** 24 + 1, 1, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 2 ** 24 + 1,
              C.byref(ns)) == F.ERR_INVALID
    assert fn(16, 3, 5, 4, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
    any_ = C.c_int32()
    masks = (C.c_uint16 * 2)(1, 1)
    buf = (C.c_uint8 * 1)()
    assert F.lib().fr_plain_find_clear(b"abc", 3, masks, 1, 0, 2 ** 63, buf, C.byref(any_)) == F.ERR_INVALID
    # a range: only its starts; the OR over more than 16 starts is a tree
    S = F.schedule_find_clear(40, 2, 3, 30)
    assert S.level_off[1] == 27 and len(S.jobs[S.level_off[1]:S.level_off[2]]) == 2


# ------------------------------------------------------------------ plain evaluation
def py_find(content: bytes, masks, lo, hi):
    m = len(masks)
    out = []
    for p in range(lo, hi):
        ok = p + m <= len(content) and all(
            (masks[i][0] >> (content[p + i] & 15)) & 1 and (masks[i][1] >> (content[p + i] >> 4)) & 1 for i in range(m))
        out.append(int(ok))
    return out


def test_plain_find_clear_against_python():
    """200 seeded random (content, needle, range) cases, lengths 1..24: content bytes over the
    whole 0..255 range (half of the cases: 0x00, bytes >= 0x80 and letters of both cases, so
    that needles recur), literals, case-insensitive letters and wildcards, partial ranges and
    ranges past the end; every start and the OR, and fr_plain_find's answers on the same inputs"""
    rng = random.Random(20250917)
    hits = 0
    for case in range(200):
        n, m = rng.randint(1, 24), min(rng.randint(1, 24), rng.randint(1, 24))
        alphabet = bytes(range(256)) if case % 2 else b"\x00aA\xe9\xc9\xff"
        content = bytes(rng.choice(alphabet) for _ in range(n))
        if rng.random() < 0.7 and m <= n:  # a needle cut from the content, so that matches occur
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
        hi = rng.randint((lo + n) // 2, n + 2)  # (past the end: starts that cannot fit)
        masks = F.needle_masks(bytes(needle), ignore_case, "?" if wild else None)
        starts, any_ = F.plain_find_clear(content, masks, lo, hi)
        want = py_find(content, masks, lo, hi)
        assert starts == want, (case, content, bytes(needle), ignore_case, wild, lo, hi)
        assert any_ == int(any(want)), case
        assert (starts, any_) == F.plain_find(content, masks, lo, hi), case
        if not ignore_case and not wild:
            assert starts == [int(content.find(bytes(needle), p, p + m) == p) for p in range(lo, hi)], case
        hits += any_
    assert 40 < hits < 180  # both answers occur often


# ------------------------------------------------------------------ the needle-length limits
@pytest.mark.parametrize("m", nl.LENGTHS)
def test_plain_find_clear_at_the_length_limits(m):
    """fr_plain_find_clear against py_starts on needle_limits.TEXT, as
    tests/test_private_needle.py does for fr_plain_find; each of the 2 m terms is read"""
    assert nl.check_plain(F.plain_find_clear, m) == nl.known_starts(m)[0]
    nl.check_every_test_counts(F.plain_find_clear, m)


@pytest.mark.parametrize("m", nl.LENGTHS)
@pytest.mark.parametrize("starts", [False, True])
def test_schedule_at_the_length_limits(m, starts):
    """fr_schedule_find_clear's jobs per level and level count from balanced_chunks(2 m) and
    or_tree: a sign gate of offset 1 - 2 len over each chunk's sum, a sum of its own each"""
    n = len(nl.TEXT)
    for lo, hi in ((0, n), (n - m - 1, n - m + 1), (n - m, n), (n - m + 1, n)):
        S = F.schedule_find_clear(n, m, lo, hi, starts=starts)
        fit = len(range(lo, min(hi, n - m + 1)))
        lvl1 = nl.check_levels(S, m, fit, starts, clear=True)
        assert all(j.kind == F.JOB_SIGN for j in S.jobs)
        made = {j.out_gate[0] for j in S.jobs}
        sums = [j.in_ref[0] for j in lvl1]
        assert all(g >= 0 and g not in made for g in sums) and len(set(sums)) == len(sums) == fit * len(nl.chunk_lens(m))
        assert [p[0] >= 0 for p in S.parts] == ([True] * fit + [False] * (hi - lo - fit) if starts else [fit > 0])


@pytest.mark.parametrize("pid", list(POINTS))
def test_oracle_alone_at_64_characters(request, key_blob, pid):
    """The reference alone is right at the longest needle: Oracle.run_schedule on find_clear and
    find_clear_starts of m = 64 over 66 bytes (three starts, eight sums of 16 terms each, an AND
    of 8 and the OR), its sums from extract_sum over an encrypted needle's 128 selectors, decodes
    to py_starts, every output's phase error below 2^53 (the bound of
    tests/test_find_clear_gpu.py's check_outputs).  Measured on 8 threads, both needles: 1.2 s at
    (1, 2048), 1.0 s at (2, 1024), plus the oracle's key generation where this test runs first
    (5 s): not marked slow."""
    import selector_cases as sc
    import test_gate_programs as tg
    k, N = POINTS[pid]
    O = tg.oracle(request, pid)
    ctx = F.Context(device=-1, params=F.default_params(k=k, N=N, ring=F.RING_FFT))
    ctx.load_client_key(key_blob)
    text = nl.DEVICE_TEXT[64]
    assert len(text) - 64 + 1 == 3
    t0 = time.perf_counter()
    for name, masks in nl.cases(64, text):
        if name not in ("plain", "absent"):
            continue
        sel = ctx.expand_needle(ctx.encrypt_needle(masks, K))
        assert sel.shape == (128, k + 1, N)
        words = np.concatenate([sc.oracle_find(O, sel, 64, text=text), sc.oracle_find(O, sel, 64, text=text, starts=True)])
        want = nl.starts_of(text, masks)
        assert want == ([2] if name == "plain" else [])
        bits = [int(bool(want))] + [int(p in want) for p in range(len(text))]
        assert [int(v) for v in O.decode16(words)] == bits, (pid, name)
        err = (O.phase(words) - (np.array(bits, dtype=U) << U(59))).view(np.int64)
        worst = int(np.abs(err).max())
        print("%s %s: largest phase error 2^%.1f" % (pid, name, np.log2(max(worst, 1))))
        assert worst < 2 ** 53, np.log2(worst)
    print("oracle %s find_clear m = 64 over 66 bytes, two needles: %.2f s" % (pid, time.perf_counter() - t0))


# ------------------------------------------------------------------ extraction
class Setup:
    def __init__(self, pid, key_blob, fixture_key):
        self.k, self.N = POINTS[pid]
        self.ctx = F.Context(device=-1, params=F.default_params(k=self.k, N=self.N, ring=F.RING_FFT))
        self.ctx.load_client_key(key_blob)
        # (phases under the big key only: no server key is generated)
        self.O = of.Oracle(fixture_key, seed=42, k=self.k, N=self.N, with_bsk=False, ring=of.RING_FFT)
        self.sel = self.ctx.expand_needle(self.ctx.encrypt_needle([(TABLES[0], TABLES[1]), (TABLES[2], TABLES[3])], K))
        # the error of every coefficient of every selector's phase
        self.err = np.stack([(self.ctx.packed_phase(self.sel[q].reshape(-1)) - direct_poly(self.N, t)).view(np.int64)
                             for q, t in enumerate(TABLES)])


@pytest.fixture(scope="module", params=list(POINTS))
def su(request, key_blob, fixture_key):
    return Setup(request.param, key_blob, fixture_key)


def test_extract_is_an_lwe_of_the_table_bit(su):
    """for every table and every nibble v, in both halves of the byte: the extracted LWE's phase
    under the flattened key is ((table >> v) & 1) 2^59 plus exactly the error of coefficient
    v N/16 of the selector's phase"""
    assert su.sel[:, :-1].any() and np.abs(su.err).max() < 2 ** 16 and su.err.any()
    for q, table in enumerate(TABLES):
        for v in range(16):
            for h, byte in ((0, v | 0xA0), (1, (v << 4) | 0x05)):
                lwe = extract_sum(su.sel, bytes([0x33, byte]), [(q, 1, h)])
                want = U(((table >> v) & 1) << 59)
                err = int((su.O.phase(lwe) - want).view(np.int64)[0])
                assert err == int(su.err[q, v * su.N // 16]), (q, v, h)


def test_sum_of_sixteen_extracts(su):
    """a 16-term sum's phase is the count of accepted nibbles times 2^59 plus an error no larger
    than the sum of its terms' errors (the triangle inequality: extraction is linear)"""
    content = bytes([0x00, 0x5F, 0xF4, 0x66, 0xFF, 0x45, 0x50, 0x6A])
    terms = [(i % 4, i // 2, i % 2) for i in range(16)]
    nib = [(content[pos] >> (4 * h)) & 15 for q, pos, h in terms]
    count = sum((TABLES[q] >> v) & 1 for (q, _, _), v in zip(terms, nib))
    assert 0 < count < 16
    lwe = extract_sum(su.sel, content, terms)
    err = int((su.O.phase(lwe) - U((count << 59) % 2 ** 64)).view(np.int64)[0])
    parts = [int(su.err[q, v * su.N // 16]) for (q, _, _), v in zip(terms, nib)]
    assert err == sum(parts)  # exactly, and therefore
    assert abs(err) <= sum(abs(e) for e in parts)


# ------------------------------------------------------------------ header, symbols, refusals
NEW = ["fr_find_clear", "fr_find_clear_starts", "fr_schedule_find_clear", "fr_plain_find_clear", "fr_dev_select_sum"]


def test_header_and_symbols():
    syms = F.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(F.lib(), name), name


def test_refusals_on_a_host_only_context(key_blob):
    c = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_FFT))
    c.load_client_key(key_blob)
    needle = C.create_string_buffer(256)  # never read: a host-only context has no needle to give
    nd = C.cast(needle, C.c_void_p)
    out = (C.c_uint32 * 4)()
    for fn in (F.lib().fr_find_clear, F.lib().fr_find_clear_starts):
        assert fn(c.h, b"abcd", 4, nd, 0, 4, out, None) == F.ERR_NO_DEVICE
        assert fn(c.h, None, 4, nd, 0, 4, out, None) == F.ERR_INVALID  # NULL content with n_chars > 0
        assert fn(c.h, b"abcd", 4, nd, 3, 2, out, None) == F.ERR_INVALID  # lo > hi
        assert fn(c.h, b"abcd", 4, None, 0, 4, out, None) == F.ERR_INVALID
    terms = (C.c_int32 * 3)(0, 0, 0)
    counts = (C.c_int32 * 1)(1)
    words = np.zeros(2049, dtype=U)
    assert F.lib().fr_dev_select_sum(c.h, nd, b"a", 1, terms, counts, 1, F._p(words)) == F.ERR_NO_DEVICE
    ms = C.c_double()
    assert F.lib().fr_dev_select_sum_ms(c.h, C.byref(ms)) == F.ERR_NO_DEVICE
