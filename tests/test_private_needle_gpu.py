"""Private search on the device: the selector variant of every blind-rotation shape
(k_blind_rotate_fft_acc), encrypted selectors, fr_find / fr_find_starts end to end, the plan
cache, lanes and the needle's release, and the refusals.

The kernel is pinned to the oracle word for word with trivial selectors (zero masks, body V(lut):
Oracle.blind_rotate) and with real ones (uniform mask words: Oracle.blind_rotate_acc, the f64
ladder from a caller's GLWE, itself pinned on the CPU by tests/test_selector_oracle.py): launches
of 1, 2, 3 and 64 jobs whose pair workgroups hold different selectors, the blind rotation's edge
rows, and one step against the exact ladder.  Whole finds are compared output by output with
Oracle.run_schedule on the same content LWEs and the needle's expanded selectors, which pins the
selector index the plan gives every job and every level above the first.

The launch shape follows the job count, so small launches are forced into every shape with the
environment switches a context reads at creation, one context per setting (shared with
tests/test_gate_programs.py where the setting is one of its own)."""
import ctypes as C

import numpy as np
import pytest

import fheregex as F
import gate_programs as gp
import selector_cases as sc
import test_gate_programs as tg  # its oracles and contexts, computed once for both
from test_exact_br import ONE_STEP_BOUND, one_step_inputs, word_gap

pytestmark = pytest.mark.gpu

U = np.uint64
# (point, environment): every shape launch_br_fft dispatches to by count
SHAPES = {
    "k1-latency": ("k1n2048", {}),
    "k1-pair": ("k1n2048", {"FR_FFT_SMALL_BATCH": 0}),
    "k1-throughput-e4": ("k1n2048", {"FR_FFT_SMALL_BATCH": 0, "FR_FFT_PAIR_BATCH": 0}),
    "k2-latency": ("k2n1024", {}),
    "k2-throughput-e8": ("k2n1024", {"FR_FFT_SMALL_BATCH": 0}),
    "k2-throughput-e4": ("k2n1024", {"FR_FFT_SMALL_BATCH": 0, "FR_FFT_LANE_ELEMS": 4}),
}
_INPUTS, _NIBBLES, _REAL, _EDGE_ACC, _ONE_STEP = {}, {}, {}, {}, {}


def direct_poly(N, lut):
    """V(lut) of test_poly<N>(t, direct = true, lut)"""
    mm = (np.arange(N) + N // 32) // (N // 16)
    return np.array([int(lut[s]) << 59 if s < 16 else -(int(lut[0]) << 59) % 2 ** 64 for s in mm], dtype=U)


def trivial_selectors(k, N, luts):
    """zero masks, body V(lut), no noise: [len(luts)][k + 1][N]"""
    acc = np.zeros((len(luts), k + 1, N), dtype=U)
    for q, lut in enumerate(luts):
        acc[q, k] = direct_poly(N, lut)
    return acc


def inputs(request, pid):
    """8 keyswitched fresh encryptions with 8 random LUTs, a ninth row with idle steps (zeroed
    mask pairs at the first step, the last step and a run), and the oracle's rows"""
    if pid not in _INPUTS:
        O = tg.oracle(request, pid)
        rng = np.random.default_rng(311)
        ks = O.keyswitch(O.encrypt_blocks(rng.integers(0, 16, 9), seed=312))
        luts = rng.integers(0, 16, (9, 16), dtype=np.uint8)
        last = (O.n + 1) // 2 - 1
        for t in (0, last, 100, 101, 102, 103):
            ks[8, 2 * t:2 * t + 2] = 0
        want = np.stack([O.blind_rotate(ks[q], list(luts[q])) for q in range(9)])
        _INPUTS[pid] = ks, luts, want
    return _INPUTS[pid]


def ctx_of(key_blob, monkeypatch, shape):
    pid, env = SHAPES[shape]
    return pid, tg.device_ctx(key_blob, monkeypatch, pid, env)


# ------------------------------------------------------------------ the kernel, pinned to the oracle
@pytest.mark.parametrize("shape", list(SHAPES))
def test_trivial_selector_is_the_lut_rotation_word_for_word(request, key_blob, monkeypatch, shape):
    """A trivial selector through fr_dev_blind_rotate_acc equals O.blind_rotate(ks, lut) word for
    word: batches of 1, 2 and 3 (the pair shape's odd tail) and all 8, then the input with idle
    steps alone, in a pair and as a tail.  Pins the ACC prologue and everything after it."""
    pid, c = ctx_of(key_blob, monkeypatch, shape)
    ks, luts, want = inputs(request, pid)
    acc = trivial_selectors(c.params.k, c.params.N, luts)
    for lo, hi in ((0, 1), (1, 3), (3, 6), (0, 8), (8, 9), (7, 9), (6, 9)):
        got = c.dev_blind_rotate_acc(ks[lo:hi], acc[lo:hi])
        bad = [q for q in range(lo, hi) if not (got[q - lo] == want[q]).all()]
        assert not bad, (shape, lo, hi, bad)
        # and the LUT launch of the same shape gives these words too
        assert np.array_equal(c.dev_blind_rotate(ks[lo:hi], luts[lo:hi]), got), (shape, lo, hi)


# ------------------------------------------------------------------ encrypted selectors
TABLES = [1 << 5, (1 << 4) | (1 << 6), 0xFFFF, 0]  # one bit, two bits, all ones, none
NIBBLE_SEED = 401  # asserted below: every input's switched phase lies inside its box


def nibbles(request, pid):
    """16 fresh nibble encryptions (values 0..15), keyswitched by the oracle; checked on the CPU:
    the phase of the modulus-switched LWE under the small key lies inside the value's box"""
    if pid not in _NIBBLES:
        O = tg.oracle(request, pid)
        N, n = O.P.N, O.n
        ks = O.keyswitch(O.encrypt_blocks(list(range(16)), seed=NIBBLE_SEED))
        log2n2 = int(np.log2(2 * N))
        sw = (((ks >> U(64 - log2n2 - 1)) + U(1)) >> U(1)) & U(2 * N - 1)  # mod_switch (common.h)
        s = np.asarray(O.s_small, dtype=U)
        phase = (sw[:, n].astype(np.int64) - (sw[:, :n] * s).sum(axis=1).astype(np.int64)) % (2 * N)
        box = N // 16
        inside = [(int(phase[v]) + box // 2) % (2 * N) // box == v for v in range(16)]
        assert all(inside), ("seed %d puts a switched phase outside its box: choose another" % NIBBLE_SEED, inside)
        _NIBBLES[pid] = ks
    return _NIBBLES[pid]


def real_selector_launches(request, c, pid):
    """(the 4 selectors of TABLES, [(keyswitched rows, one selector per row, the oracle's rows)]),
    once per point.  The first launch is the 64 jobs of test_encrypted_selectors; then 1, 2 and 3
    nibble jobs and the idle-step row of inputs() alone, in a pair and as the odd tail, the jobs
    of every pair workgroup on different selectors."""
    if pid not in _REAL:
        O = tg.oracle(request, pid)
        nib = nibbles(request, pid)
        ks9 = inputs(request, pid)[0]
        sel = c.expand_needle(c.encrypt_needle([(TABLES[0], TABLES[1]), (TABLES[2], TABLES[3])], seed=402))
        launches = [(np.tile(nib, (4, 1)), np.repeat(sel, 16, axis=0))]
        for rows, which in ((nib[[5]], [0]), (nib[[5, 6]], [1, 2]), (nib[[9, 5, 14]], [3, 0, 2]),
                            (ks9[[8]], [1]), (ks9[[7, 8]], [0, 2]), (ks9[[6, 7, 8]], [3, 1, 2])):
            assert all(a != b for a, b in zip(which[0::2], which[1::2]))
            launches.append((rows, sel[which]))
        _REAL[pid] = sel, [(ks, acc, O.blind_rotate_acc(ks, acc)) for ks, acc in launches]
    return _REAL[pid]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_encrypted_selectors(request, key_blob, monkeypatch, shape):
    """16 nibbles against one encrypted selector per table, one launch of 64 jobs per shape: every
    output decrypts to lut[nibble], and its phase error is below 2^53, the bound
    tests/test_noise.py holds bootstrap outputs to (the selector's fresh noise adds 2^12.4).
    And every word of every output equals Oracle.blind_rotate_acc's, in that launch and in
    launches of 1, 2 and 3 jobs (the pair shape's odd tail) whose pair workgroups hold two
    different selectors, with and without idle steps: the prologue's load, rotation and sign of
    the mask polynomials, the polynomial index at k = 2 and the per-job selector pointer."""
    pid, c = ctx_of(key_blob, monkeypatch, shape)
    O = tg.oracle(request, pid)
    ks = nibbles(request, pid)
    sel, launches = real_selector_launches(request, c, pid)
    assert sel[:, :-1].any()  # real masks
    got = c.dev_blind_rotate_acc(np.tile(ks, (4, 1)), np.repeat(sel, 16, axis=0))
    for at, (rows, accs, words) in enumerate(launches):
        dev = got if at == 0 else c.dev_blind_rotate_acc(rows, accs)
        bad = [q for q in range(len(rows)) if not np.array_equal(dev[q], words[q])]
        assert not bad, (shape, "launch %d of %d jobs" % (at, len(rows)), bad[:12])
    want = np.array([(t >> v) & 1 for t in TABLES for v in range(16)], dtype=U)
    assert list(O.decode16(got)) == list(want), shape
    err = (O.phase(got) - (want << U(59))).view(np.int64)
    worst = int(np.abs(err).max())
    print("%s: largest phase error 2^%.1f" % (shape, np.log2(max(worst, 1))))
    assert worst < 2 ** 53, (shape, np.log2(worst))


def edge_selectors(request, pid):
    """the unique edge rows of gate_programs.edge_rows, a uniform-random accumulator with the
    planted words of selector_cases for each, and the oracle's rows"""
    if pid not in _EDGE_ACC:
        O = tg.oracle(request, pid)
        names, ks, _, _ = tg.edge(request, pid)
        acc = sc.random_accs(len(names), O.P.k, O.P.N, seed=83)
        _EDGE_ACC[pid] = names, ks, acc, O.blind_rotate_acc(ks, acc)
    return _EDGE_ACC[pid]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_edge_rows_with_a_real_selector(request, key_blob, monkeypatch, shape):
    """The mask and body edge rows (idle ladders and pairs, exponents that cancel, rounding ties,
    bodies on box boundaries and the wrap body) from full-magnitude accumulators that hold the
    conversion's edge words in every polynomial, word for word against Oracle.blind_rotate_acc.
    The pair shape runs them behind the workgroup pairs of gate_programs.EDGE_HEAD."""
    pid, c = ctx_of(key_blob, monkeypatch, shape)
    names, ks, acc, words = edge_selectors(request, pid)
    order = gp.edge_order(names, 41) if shape == "k1-pair" else list(range(len(names)))
    got = c.dev_blind_rotate_acc(ks[order], acc[order])
    bad = [(i, names[u]) for i, u in enumerate(order) if not np.array_equal(got[i], words[u])]
    assert not bad, (shape, len(bad), bad[:12])


def one_step_selectors(request, pid):
    """24 one-step ladders from uniform-random accumulators: the exact ladder's and the f64
    ladder's rows"""
    if pid not in _ONE_STEP:
        O = tg.oracle(request, pid)
        ks, _ = one_step_inputs(O, 24, seed=91)
        acc = sc.random_accs(24, O.P.k, O.P.N, seed=92)
        _ONE_STEP[pid] = ks, acc, O.blind_rotate_exact(ks, accs=acc), O.blind_rotate_acc(ks, acc)
    return _ONE_STEP[pid]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_one_step_from_a_selector_against_exact(request, key_blob, monkeypatch, shape):
    """tests/test_exact_br.py's test_device_one_step_against_exact from full-magnitude
    accumulators: every output word of the device within 2^44 (DESIGN §2.1's per-product bound)
    of the exact ladder's, which rotates the accumulator in u64 with no rounding; and equal to
    the f64 ladder's."""
    pid, c = ctx_of(key_blob, monkeypatch, shape)
    ks, acc, exact, f64 = one_step_selectors(request, pid)
    dev = c.dev_blind_rotate_acc(ks, acc)
    worst = max(word_gap(dev[q], exact[q]) for q in range(len(ks)))
    print("%s: max |device - exact| = 2^%.2f over %d one-step ladders from uniform accumulators"
          % (shape, np.log2(max(worst, 1)), len(ks)))
    assert worst <= ONE_STEP_BOUND, (shape, np.log2(worst))
    assert np.array_equal(dev, f64), shape


# ------------------------------------------------------------------ end to end
CONTENT = "xxabcxxAbCxxxxab"
NEEDLES = [("abc", False, None), ("abc", True, None), ("a?c", False, "?"), ("x", False, None),
           ("xxabcxxAb", False, None), ("zzz", False, None)]
_E2E = {}


def py_starts(content, masks):
    """content: a str (its bytes) or the bytes themselves, every value valid"""
    b, m = content.encode() if isinstance(content, str) else bytes(content), len(masks)
    return [p for p in range(len(b)) if p + m <= len(b) and all(
        (masks[i][0] >> (b[p + i] & 15)) & 1 and (masks[i][1] >> (b[p + i] >> 4)) & 1 for i in range(m))]


def e2e(key_blob, pid):
    """a context of its own per point (it gets a packing key), content uploaded once: fresh
    encryptions, and the same with its first four characters trivial"""
    if pid not in _E2E:
        k, N, ring = tg.POINTS[pid]
        c = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
        c.load_client_key(key_blob)
        c.gen_server_key(tg.SEED)
        c.gen_packing_key(9, compact=True)
        ck, sk = F.ClientKey(c), F.ServerKey(c)
        hs = ck.encrypt_str(CONTENT, seed=11)
        mixed = [sk.create_trivial_radix(ord(ch)) for ch in CONTENT[:4]] + hs[4:]
        _E2E[pid] = c, ck, sk, hs, mixed
    return _E2E[pid]


@pytest.mark.parametrize("needle", NEEDLES, ids=[n[0] + ("-i" if n[1] else "") for n in NEEDLES])
@pytest.mark.parametrize("pid", ["k1n2048", "k2n1024"])
def test_find_and_find_starts(key_blob, pid, needle):
    c, ck, sk, hs, mixed = e2e(key_blob, pid)
    s, ignore_case, any_char = needle
    want = py_starts(CONTENT, F.needle_masks(s, ignore_case, any_char))
    if not ignore_case and any_char is None:
        assert want == [p for p in range(len(CONTENT)) if CONTENT.startswith(s, p)]
    nd = sk.upload_needle(ck.encrypt_needle(s, ignore_case, any_char, seed=21))
    assert len(nd) == len(s)
    for content in (hs, mixed):
        out = sk.find(content, nd)
        assert ck.decrypt(out) == int(bool(want)), (pid, s)
        c.release(out)
        for compact in (False, True):
            assert ck.decrypt_starts(sk.find_starts(content, nd, compact=compact)) == want, (pid, s, compact)
    nd.close()


WORD_NEEDLES = ["abc", "xxabcxxAb"]  # one AND gate per start; 18 tests per start: a two-level AND


def output_words(c, handles):
    return np.stack([c.download_radix(h)[0] for h in handles])


def device_find_words(c, nd, content):
    """block 0 of fr_find's output, then of every output of fr_find_starts"""
    out, _ = c.find(content, nd)
    starts = c.find_starts(content, nd)
    try:
        return output_words(c, [out] + starts)
    finally:
        for h in [out] + starts:
            c.release(h)


def oracle_find_words(c, O, sel, m, content):
    """the same rows from Oracle.run_schedule on the handles' own LWEs and the selector table"""
    lwes = np.stack([c.download_radix(h) for h in content])
    return np.concatenate([sc.oracle_find(O, sel, m, content_lwes=lwes),
                           sc.oracle_find(O, sel, m, content_lwes=lwes, starts=True)])


@pytest.mark.parametrize("s", WORD_NEEDLES)
@pytest.mark.parametrize("pid", ["k1n2048", "k2n1024"])
def test_find_words(request, key_blob, pid, s):
    """Whole finds word for word: every output of fr_find and fr_find_starts against
    Oracle.run_schedule over the selector table fr_expand_needle gives for the same blob, on
    fresh content and on content whose first four characters are trivial."""
    c, ck, sk, hs, mixed = e2e(key_blob, pid)
    O = tg.oracle(request, pid)
    blob = ck.encrypt_needle(s, seed=21)
    sel = c.expand_needle(blob)
    nd = sk.upload_needle(blob)
    try:
        for what, content in (("fresh", hs), ("mixed", mixed)):
            got, want = device_find_words(c, nd, content), oracle_find_words(c, O, sel, len(s), content)
            assert got.shape == want.shape == (1 + len(CONTENT), c.lwe_len)
            bad = [i - 1 for i in range(len(got)) if not np.array_equal(got[i], want[i])]  # (-1: fr_find's)
            assert not bad, (pid, s, what, bad)
    finally:
        nd.close()


def test_find_words_on_two_lanes(request, key_blob):
    """the same comparison with two lanes, asynchronous: the serial run's words and the oracle's"""
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    O = tg.oracle(request, "k1n2048")
    blob = ck.encrypt_needle("abc", seed=21)
    sel = c.expand_needle(blob)
    want = oracle_find_words(c, O, sel, 3, hs)
    nd = sk.upload_needle(blob)
    try:
        serial = device_find_words(c, nd, hs)
        assert np.array_equal(serial, want)
        c.set_lanes(2)
        c.set_async(True)
        for rep in range(2):  # (the first round compiles each lane's plan copy)
            assert np.array_equal(device_find_words(c, nd, hs), serial), rep
    finally:
        c.set_lanes(1)
        nd.close()


def test_needle_longer_than_the_content_is_the_constant(key_blob):
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    nd = sk.upload_needle(ck.encrypt_needle("abcde", seed=22))
    out, st = c.find(hs[:4], nd)
    assert ck.decrypt(out) == 0 and st.pbs == 0
    c.release(out)
    starts = c.find_starts(hs[:4], nd)
    assert [ck.decrypt(h) for h in starts] == [0, 0, 0, 0]
    for h in starts:
        c.release(h)
    nd.close()


# ------------------------------------------------------------------ plan cache, lanes, release
def test_second_needle_of_the_same_length_is_a_cache_hit(key_blob):
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    a = sk.upload_needle(ck.encrypt_needle("abc", seed=31))
    b = sk.upload_needle(ck.encrypt_needle("zab", seed=32))  # no match: not a's answer
    out_a, st_a = c.find(hs, a)
    hits = c.plan_cache_stats()["hits"]
    out_b, st_b = c.find(hs, b)
    assert c.plan_cache_stats()["hits"] == hits + 1 and st_b.plan_cached == 1
    assert (ck.decrypt(out_a), ck.decrypt(out_b)) == (1, 0)
    out_a2, _ = c.find(hs, a)  # and back: the plan holds nothing of b
    assert ck.decrypt(out_a2) == 1
    for h in (out_a, out_b, out_a2):
        c.release(h)
    a.close(), b.close()


def test_lanes_and_release(key_blob):
    """With two lanes, four consecutive asynchronous finds give the one-lane result words bit for
    bit; freeing the needle right after them waits for the lanes, and arena and handle counts
    return to where they started once the results are released."""
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    blob = ck.encrypt_needle("abc", seed=41)
    nd = sk.upload_needle(blob)
    first, _ = c.find(hs, nd)
    one = c.download_radix(first)
    c.release(first)
    nd.close()
    c.set_lanes(2)
    try:
        warm = sk.upload_needle(blob)
        outs = [c.find(hs, warm)[0] for _ in range(2)]  # each lane's plan copy, cached
        for h in outs:
            c.download_radix(h)
            c.release(h)
        warm.close()
        arena = c.arena_stats()
        handles = c.handle_count()
        nd = sk.upload_needle(blob)
        outs = [c.find(hs, nd)[0] for _ in range(4)]
        nd.close()  # asynchronous finds may still be queued: the release waits for every lane
        words = [c.download_radix(h) for h in outs]
        for w in words:
            assert np.array_equal(w, one)
        for h in outs:
            c.release(h)
        after = c.arena_stats()  # (synchronises every lane: deferred frees return)
        assert after["slots"] - after["free_slots"] == arena["slots"] - arena["free_slots"]
        assert c.handle_count() == handles
    finally:
        c.set_lanes(1)


# ------------------------------------------------------------------ refusals
def find_rc(c, hs, needle_h):
    arr = (C.c_uint32 * len(hs))(*hs)
    out = (C.c_uint32 * len(hs))()
    return (F.lib().fr_find(c.h, arr, len(hs), needle_h, 0, len(hs), out, None),
            F.lib().fr_find_starts(c.h, arr, len(hs), needle_h, 0, len(hs), out, None))


def test_refusals(key_blob, monkeypatch):
    """an error code each, and nothing planned or launched"""
    c1, ck1, sk1, hs1, _ = e2e(key_blob, "k1n2048")
    c2, ck2, sk2, hs2, _ = e2e(key_blob, "k2n1024")
    n1 = sk1.upload_needle(ck1.encrypt_needle("abc", seed=51))
    n2 = sk2.upload_needle(ck2.encrypt_needle("abc", seed=52))
    h = C.c_void_p()
    # an RNS context: no upload, no find
    rns = tg.device_ctx(key_blob, monkeypatch, "rns", {})
    blob = ck1.encrypt_needle("abc", seed=51)
    assert F.lib().fr_upload_needle(rns.h, blob, len(blob), C.byref(h)) == F.ERR_INVALID
    assert "FFT ring only" in F.lib().fr_last_error().decode()
    rhs = rns.upload_radix(rns.encrypt_str("abcd", seed=1))
    before = rns.plan_cache_stats(), rns.arena_stats()
    assert find_rc(rns, rhs, n1.h) == (F.ERR_INVALID, F.ERR_INVALID)
    assert "FFT ring only" in F.lib().fr_last_error().decode()
    assert (rns.plan_cache_stats(), rns.arena_stats()) == before
    for x in rhs:
        rns.release(x)
    # a needle of another (k, N), both ways; a blob of another (k, N)
    for c, hs, other in ((c1, hs1, n2), (c2, hs2, n1)):
        before = c.plan_cache_stats(), c.arena_stats()
        assert find_rc(c, hs, other.h) == (F.ERR_INVALID, F.ERR_INVALID)
        assert (c.plan_cache_stats(), c.arena_stats()) == before
    assert F.lib().fr_upload_needle(c2.h, blob, len(blob), C.byref(h)) == F.ERR_INVALID
    # a needle of the same (k, N) uploaded to another context
    other = tg.device_ctx(key_blob, monkeypatch, "k1n2048", {})
    ohs = other.upload_radix(other.encrypt_str("abcd", seed=1))
    assert find_rc(other, ohs, n1.h) == (F.ERR_INVALID, F.ERR_INVALID)
    for x in ohs:
        other.release(x)
    # a host-only context
    host = F.Context(device=-1, params=c1.params)
    host.load_client_key(key_blob)
    assert F.lib().fr_upload_needle(host.h, blob, len(blob), C.byref(h)) == F.ERR_NO_DEVICE
    assert find_rc(host, [0], n1.h) == (F.ERR_NO_DEVICE, F.ERR_NO_DEVICE)
    n1.close(), n2.close()


def test_needle_free_takes_its_own_context(key_blob, monkeypatch):
    c1, ck1, sk1, _, _ = e2e(key_blob, "k1n2048")
    other = tg.device_ctx(key_blob, monkeypatch, "k1n2048", {})
    nd = sk1.upload_needle(ck1.encrypt_needle("ab", seed=61))
    assert F.lib().fr_needle_free(other.h, nd.h) == F.ERR_INVALID
    assert len(nd) == 2  # nothing was freed
    assert F.lib().fr_needle_free(c1.h, None) == F.FR_OK
    nd.close()


def test_find_cuts_its_range_at_the_content(key_blob):
    """start_hi far past the content: the same answer, the same plan, and no walk over the range"""
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    nd = sk.upload_needle(ck.encrypt_needle("abc", seed=62))
    a, _ = c.find(hs, nd)
    hits = c.plan_cache_stats()["hits"]
    b, st = c.find(hs, nd, 0, 2 ** 63)
    assert c.plan_cache_stats()["hits"] == hits + 1 and st.plan_cached == 1
    assert (ck.decrypt(a), ck.decrypt(b)) == (1, 1)
    out = (C.c_uint32 * 1)()
    arr = (C.c_uint32 * len(hs))(*hs)
    assert F.lib().fr_find_starts(c.h, arr, len(hs), nd.h, 0, 2 ** 63, out, None) == F.ERR_INVALID
    for h in (a, b):
        c.release(h)
    nd.close()


# ------------------------------------------------------------------ the hooks' timers
@pytest.mark.parametrize("lanes", [1, 2])
def test_profiled_hooks_then_profiled_matches(request, key_blob, lanes):
    """Under fr_set_profiling the parity hooks stamp two events where a level stamps up to four.
    Profiling on, each hook, then profiled matches and finds on the same context (with lanes:
    asynchronous ones still queued when the next hook resolves the timers): every call succeeds,
    the timers count each launch once, and the results are right."""
    c, ck, sk, hs, _ = e2e(key_blob, "k1n2048")
    ks, luts, want = inputs(request, "k1n2048")
    acc = trivial_selectors(c.params.k, c.params.N, luts)
    nd = sk.upload_needle(ck.encrypt_needle("abc", seed=63))
    c.set_lanes(lanes)
    try:
        for level in (1, 2):
            c.set_profiling(level)
            t0 = c.device_timers()
            for rep in range(3):
                assert np.array_equal(c.dev_blind_rotate(ks[:2], luts[:2]), want[:2])
                assert np.array_equal(c.dev_blind_rotate_acc(ks[2:5], acc[2:5]), want[2:5])
                assert np.array_equal(c.dev_blind_rotate_multi(ks[5], luts[5:6], direct=True)[0], want[5])
                m, st_m = c.has_match(hs, "/abc/")
                f, st_f = c.find(hs, nd)
                f2, _ = c.find(hs, nd)
                assert [ck.decrypt(h) for h in (m, f, f2)] == [1, 1, 1]  # (a download: every timer resolves)
                for h in (m, f, f2):
                    c.release(h)
            t1 = c.device_timers()
            launches = 3 * (3 + int(st_m.levels) + 2 * int(st_f.levels))
            assert t1["br_launches"] - t0["br_launches"] == launches, (level, lanes)
            assert t1["br_gates"] - t0["br_gates"] == 3 * (2 + 3 + 1 + int(st_m.blind_rotations)
                                                           + 2 * int(st_f.blind_rotations))
            assert t1["br_ms"] > t0["br_ms"]
    finally:
        c.set_profiling(0)
        c.set_lanes(1)
        nd.close()
