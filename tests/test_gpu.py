"""GPU parity tests (MI355X): every kernel stage bit-exact against the CPU
oracle on the same keys and inputs; decrypted match results equal to the
reference's (plaintext oracle + the reference's own 25 vectors)."""
import json
import os

import numpy as np
import pytest

import fheregex as F
import oracle_ffi as of
import regex_oracle as ro
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED = 42


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


# (ring, k, N): the reference's parameters and BASELINE's "N = 1024" set (k = 2,
# N = 1024) on the FFT ring (the product path), and the opt-in RNS/NTT ring (DESIGN.md
# §2.1) at the reference's parameters.  The RNS point runs every test by default except the
# word-for-word whole-match comparisons whose oracle side is slow on that ring
# (tests/conftest.py RNS_HEAVY, ~11 of the 12 minutes of its full matrix); FR_TEST_RNS=1
# runs those too.
POINTS = [(F.RING_FFT, 1, 2048), (F.RING_FFT, 2, 1024), (F.RING_RNS, 1, 2048)]
POINT_IDS = ["fft", "fft-k2n1024", "rns"]


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def gctx(request, key_blob):
    """Every test below runs at every point."""
    ring, k, N = request.param
    ctx = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    return ctx


@pytest.fixture(scope="module")
def oracle_k1(gctx, fixture_key):
    """Oracle keys at the context's point (server-key seed 42)."""
    p = gctx.params
    return of.Oracle(fixture_key, seed=SEED, k=p.k, N=p.N, ring=p.ring)


def test_device_info(gctx):
    assert "gfx950" in gctx.info()


def test_ring_mul_bit_exact(key_blob):
    """the RNS ring's product test hook (the FFT product is covered by tests/test_fft.py)"""
    gctx = F.Context(device=0, params=F.default_params(k=1, N=2048, ring=F.RING_RNS))
    rng = np.random.default_rng(1)
    P = of.Q_RING
    a = rng.integers(0, P, (3, 2048), dtype=np.uint64)
    b = rng.integers(0, P, (3, 2048), dtype=np.uint64)
    b[1] = 0
    b[1][5] = 1  # X^5
    b[2] = np.array([int(d) % P for d in rng.integers(-(1 << 22), 1 << 22, 2048)], dtype=np.uint64)  # digit-sized
    got = gctx.dev_ring_mul(a, b)
    for i in range(3):
        exp = np.zeros(2048, np.uint64)
        of.lib().or_ring_mul(2048, of.ptr(np.ascontiguousarray(a[i])), of.ptr(np.ascontiguousarray(b[i])), of.ptr(exp))
        assert (got[i] == exp).all(), i


def test_keyswitch_bit_exact(gctx, oracle_k1):
    O = oracle_k1
    blocks = O.encrypt_blocks([3, 7, 0, 15, 9, 1, 2, 12, 4, 5, 6, 8, 10, 11, 13, 14, 3, 3, 3, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13],
                              seed=77)
    got = gctx.dev_keyswitch(blocks)
    exp = O.keyswitch(blocks)
    assert got.shape == exp.shape
    assert (got == exp).all()


@pytest.mark.parametrize("count", [1, 32, 33, 95, 96, 97, 100, 129, 130, 300, 600])
def test_keyswitch_batch_sizes_bit_exact(gctx, oracle_k1, count):
    """MFMA keyswitch paths (fragment-ordered operands): one row tile per wave with
    8 K slices (1; 32: one full tile; 33: the first padded second tile; 95: the last
    batch below FR_KS_MR4_MIN); the LDS-DMA four-row-tile kernel with padding rows: 5 K
    slices (96, 97: at and past the threshold; 100 -> 128 rows; 129, 130 -> 256 rows: the
    second 128-row group), 2 (300 -> 384 rows) and 1 (600 -> 640 rows); random
    (non-message) masks."""
    rng = np.random.default_rng(count)
    blocks = rng.integers(0, 2**64 - 1, (count, gctx.lwe_len), dtype=np.uint64, endpoint=True)
    got = gctx.dev_keyswitch(blocks)
    exp = oracle_k1.keyswitch(blocks)
    assert (got == exp).all()


def test_keyswitch_two_column_tiles_bit_exact(key_blob, fixture_key, monkeypatch):
    """The FR_KS_MC=2 keyswitch shape (two column tiles per wave; opt-in) and a forced
    K split (FR_KS_SPLIT=10), bit-exact against the oracle."""
    monkeypatch.setenv("FR_KS_MC", "2")
    monkeypatch.setenv("FR_KS_SPLIT", "10")
    ctx = F.Context(device=0)
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    O = of.Oracle(fixture_key, seed=SEED)
    rng = np.random.default_rng(600)
    blocks = rng.integers(0, 2**64 - 1, (600, ctx.lwe_len), dtype=np.uint64, endpoint=True)
    assert (ctx.dev_keyswitch(blocks) == O.keyswitch(blocks)).all()


def test_keyswitch_byte_store_digit_pass_bit_exact(key_blob, fixture_key, monkeypatch):
    """The digit pass with per-digit byte stores (FR_KS_DIG16=0; the default writes each
    thread's 16 coefficients as whole 16-byte fragment pieces) gives the oracle's words."""
    monkeypatch.setenv("FR_KS_DIG16", "0")
    ctx = F.Context(device=0)
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    O = of.Oracle(fixture_key, seed=SEED)
    rng = np.random.default_rng(300)
    blocks = rng.integers(0, 2**64 - 1, (300, ctx.lwe_len), dtype=np.uint64, endpoint=True)
    assert (ctx.dev_keyswitch(blocks) == O.keyswitch(blocks)).all()


@pytest.mark.parametrize("count", [1, 17, 600])
def test_keyswitch_plain_workgroup_order_bit_exact(key_blob, fixture_key, monkeypatch, count):
    """The keyswitch GEMM's plain workgroup order (FR_KS_XCD=0; the default deals
    column groups to XCDs) gives the oracle's words too, with one and four row tiles
    per wave."""
    monkeypatch.setenv("FR_KS_XCD", "0")
    ctx = F.Context(device=0)
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    O = of.Oracle(fixture_key, seed=SEED)
    rng = np.random.default_rng(count + 1)
    blocks = rng.integers(0, 2**64 - 1, (count, ctx.lwe_len), dtype=np.uint64, endpoint=True)
    assert (ctx.dev_keyswitch(blocks) == O.keyswitch(blocks)).all()


def test_blind_rotate_bit_exact(gctx, oracle_k1):
    O = oracle_k1
    blocks = O.encrypt_blocks([5, 12, 0], seed=31)
    ks = O.keyswitch(blocks)
    luts = [[(3 * m + 1) % 16 for m in range(16)], [int(m >= 4) for m in range(16)], [m ^ 5 for m in range(16)]]
    got = gctx.dev_blind_rotate(ks, luts)
    for i in range(3):
        exp = O.blind_rotate(ks[i], luts[i])
        assert (got[i] == exp).all(), i
        assert O.decode16(got[i])[0] == luts[i][[5, 12, 0][i]]


def test_multi_value_blind_rotate_bit_exact(gctx, oracle_k1):
    O = oracle_k1
    ks = O.keyswitch(O.encrypt_blocks([6, 13], seed=55))
    luts = [[int(v == 6) for v in range(16)], [int(v in (6, 13)) for v in range(16)], [int(v >= 9) for v in range(16)],
            [int(v == 13) for v in range(16)], [int(v % 2 == 0) for v in range(16)]]
    for i, m in enumerate([6, 13]):
        got = gctx.dev_blind_rotate_multi(ks[i], luts)
        exp = O.blind_rotate_multi(ks[i], luts)
        assert (got == exp).all(), i
        assert [int(O.decode16(o)[0]) for o in got] == [l[m] for l in luts]


def test_executor_merges_same_input_gates(gctx):
    rng = np.random.default_rng(12)
    s = "".join(chr(c) for c in rng.integers(0x20, 0x7F, 40))
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=12))
    out, st = gctx.has_match(hs, "/abc/")
    assert st.blind_rotations < st.pbs  # lo-nibble tests for a, b, c share one rotation per char
    assert gctx.decrypt_radix(gctx.download_radix(out)) == ro.has_match(s, "/abc/").result
    gctx.set_multi_value(False)
    try:
        out2, st2 = gctx.has_match(hs, "/abc/")
    finally:
        gctx.set_multi_value(True)
    assert st2.blind_rotations == st2.pbs == st.pbs
    assert gctx.decrypt_radix(gctx.download_radix(out2)) == gctx.decrypt_radix(gctx.download_radix(out))


def test_gate_program_bit_exact(gctx, oracle_k1):
    """Lincomb + KS + BR through fr_run_gates vs the oracle's gate evaluation."""
    O = oracle_k1
    s = b"Hi!"
    ct = O.encrypt_str(s, seed=3)
    hs = gctx.upload_radix(ct)
    luts = [[int(v == (0x48 & 15)) for v in range(16)], [int(v == (0x69 >> 4)) for v in range(16)]]
    gates = []
    for j, (h, half) in enumerate([(hs[0], 0), (hs[1], 1)]):
        g = F.Gate()
        g.n_in = 2
        g.offset = 0
        g.in_[0], g.in_block[0], g.in_w[0] = h, 2 * half, 1
        g.in_[1], g.in_block[1], g.in_w[1] = h, 2 * half + 1, 4
        for v in range(16):
            g.lut[v] = luts[j][v]
        gates.append(g)
    g = F.Gate()  # depends on both: [a + b == 2]
    g.n_in = 2
    g.in_[0], g.in_w[0] = 0x80000000 | 0, 1
    g.in_[1], g.in_w[1] = 0x80000000 | 1, 1
    for v in range(16):
        g.lut[v] = int(v == 2)
    gates.append(g)
    outs = gctx.run_gates(gates)
    got = np.stack([gctx.download_radix(o)[0] for o in outs])
    slots = ct.reshape(-1, ct.shape[-1])
    exp01 = O.gates([([(0, 1), (1, 4)], 0, luts[0]), ([(4 + 2, 1), (4 + 3, 4)], 0, luts[1])], slots)
    assert (got[0] == exp01[0]).all() and (got[1] == exp01[1]).all()
    exp2 = O.gates([([(0, 1), (1, 1)], 0, [int(v == 2) for v in range(16)])], exp01)
    assert (got[2] == exp2[0]).all()
    assert [int(O.decode16(got[i])[0]) for i in range(3)] == [1, 1, 1]


@pytest.mark.parametrize("v", load("engine_vectors.json"), ids=lambda v: f'{v["content"]!r}-{v["pattern"]}')
def test_reference_vectors_trivial_content(gctx, v):
    """src/regex/engine.rs:256-291 exactly as the reference runs them: trivial radix content."""
    hs = [gctx.trivial(b) for b in v["content"].encode()]
    out, st = gctx.has_match(hs, v["pattern"])
    assert gctx.decrypt_radix(gctx.download_radix(out)) == v["expected"]
    assert (st.ct_ops, st.cache_hits) == (v["ct_ops"], v["cache_hits"])


@pytest.mark.parametrize("v", load("engine_vectors.json"), ids=lambda v: f'{v["content"]!r}-{v["pattern"]}')
def test_reference_vectors_encrypted_content(gctx, v):
    hs = gctx.upload_radix(gctx.encrypt_str(v["content"], seed=len(v["content"]) + 100))
    out, st = gctx.has_match(hs, v["pattern"])
    assert gctx.decrypt_radix(gctx.download_radix(out)) == v["expected"]
    for h in hs:
        gctx.release(h)


def test_readme_semantics_encrypted(gctx):
    """The reference README's documented constructs (README.md:33-58, tests/golden/
    readme_vectors.json: 100 pattern/content cases, the two ct_ge quirk cases following the
    code) on encrypted content, each result decrypted"""
    cases = load("readme_vectors.json")["cases"]
    for i, c in enumerate(cases):
        exp = c.get("code", c["readme"])
        hs = gctx.encrypt_upload_str(c["content"], seed=500 + i) if c["content"] else []
        out, _ = gctx.has_match(hs, c["pattern"])
        assert gctx.decrypt_radix(gctx.download_radix(out)) == exp, c
        for h in hs + [out]:
            gctx.release(h)


def test_eager_ops(gctx):
    s = "aMz~ 0"
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=9))
    dec = lambda h: gctx.decrypt_radix(gctx.download_radix(h))
    for h, ch in zip(hs, s.encode()):
        for c in (ch, ch - 1, ch + 1, ord("a"), ord("M")):
            c &= 0xFF
            assert dec(gctx.eq_const(h, c)) == int(ch == c)
            assert dec(gctx.gt_const(h, c)) == int(ch > c)
            assert dec(gctx.le_const(h, c)) == int(ch <= c)
    e1, e0 = gctx.eq_const(hs[0], ord("a")), gctx.eq_const(hs[0], ord("b"))
    assert [dec(gctx.and_(x, y)) for x, y in [(e1, e1), (e1, e0), (e0, e0)]] == [1, 0, 0]
    assert [dec(gctx.or_(x, y)) for x, y in [(e1, e1), (e1, e0), (e0, e0)]] == [1, 1, 0]
    assert [dec(gctx.not_(x)) for x in (e1, e0)] == [0, 1]
    assert dec(gctx.not_(gctx.not_(e1))) == 1
    # general radix bitand / bitor / bitxor-1 on characters
    assert dec(gctx.and_(hs[0], hs[1])) == (ord("a") & ord("M"))
    assert dec(gctx.or_(hs[0], hs[1])) == (ord("a") | ord("M"))
    assert dec(gctx.not_(hs[2])) == (ord("z") ^ 1)
    assert dec(gctx.or_many([e0, e0, e1, e0])) == 1
    assert dec(gctx.or_many([e0] * 20)) == 0


def _config(gctx, content, pattern, seed):
    hs = gctx.upload_radix(gctx.encrypt_str(content, seed=seed))
    out, st = gctx.has_match(hs, pattern)
    got = gctx.decrypt_radix(gctx.download_radix(out))
    for h in hs:
        gctx.release(h)
    return got, st


def _printable(rng, n):
    return "".join(chr(c) for c in rng.integers(0x20, 0x7F, n))


def test_config1(gctx):
    got, st = _config(gctx, "abc", "/^abc$/", 1)
    assert got == 1 and (st.ct_ops, st.cache_hits) == (5, 0)


@pytest.mark.parametrize("planted", [True, False])
def test_config2_abc_64(gctx, planted):
    rng = np.random.default_rng(2)
    s = _printable(rng, 64)
    if planted:
        s = s[:17] + "abc" + s[20:]
    exp = ro.has_match(s, "/abc/")
    got, st = _config(gctx, s, "/abc/", 2)
    assert got == exp.result and st.ct_ops == exp.ct_ops == 371


@pytest.mark.parametrize("planted", [True, False])
def test_large_content_abc_4096(gctx, planted):
    """Maximum-size case: 4096 chars (16 x the metric) -> 8192 level-1 bootstraps (four
    throughput launches' worth, arena and batch growth), content encrypted on the device;
    the match bit against the plaintext oracle, op counts against the plaintext lowering."""
    rng = np.random.default_rng(44)
    s = _printable(rng, 4096).replace("abc", "abd")
    if planted:
        s = s[:4000] + "abc" + s[4003:]
    hs = gctx.encrypt_upload_str(s, seed=45)
    out, st = gctx.has_match(hs, "/abc/")
    got = gctx.decrypt_radix(gctx.download_radix(out))
    assert got == int(planted)
    pm = F.plain_match(s.encode(), "/abc/", engine=F.ENGINE_AUTO)
    assert got == pm.result_lowered and (st.ct_ops, st.levels) == (pm.ct_ops, pm.levels)
    assert st.blind_rotations >= 2 * 4096
    for h in hs + [out]:
        gctx.release(h)


def test_metric_abc_256(gctx):
    rng = np.random.default_rng(0)
    s = _printable(rng, 256)
    s = s[:200] + "abc" + s[203:]
    got, st = _config(gctx, s, "/abc/", 3)
    assert got == 1 and st.ct_ops == 1523


@pytest.mark.parametrize("hit", [True, False])
def test_pair_shape_match_bit_identical(key_blob, monkeypatch, hit):
    """/abc/ on 256 chars (its first level: 512 multi-value bootstraps) with the pair
    shape (a k = 1 geometry) on and off: the result ciphertext is the same bit for bit
    (multi-value and sign jobs through both shapes)."""
    p = F.default_params(k=1, N=2048, ring=F.RING_FFT)
    rng = np.random.default_rng(11)
    s = _printable(rng, 256).replace("abc", "abd")
    if hit:
        s = s[:77] + "abc" + s[80:]
    words = []
    for lim in (0, 4096):
        monkeypatch.setenv("FR_FFT_PAIR_BATCH", str(lim))
        c = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
        monkeypatch.delenv("FR_FFT_PAIR_BATCH")
        c.load_client_key(key_blob)
        c.gen_server_key(SEED)
        o, _ = c.has_match(c.upload_radix(c.encrypt_str(s, seed=5)), "/abc/")
        words.append(c.download_radix(o))
        assert c.decrypt_radix(words[-1]) == int(hit)
    assert (words[0] == words[1]).all()


@pytest.mark.parametrize("kind", ["letters", "digit"])
def test_config3_proxy(gctx, kind):
    rng = np.random.default_rng(4)
    s = "".join(chr(c) for c in rng.integers(ord("b"), ord("z") + 1, 256))
    if kind == "digit":
        s = s[:100] + "7" + s[101:]
    exp = ro.has_match(s, "/^[a-z]+$/")
    got, st = _config(gctx, s, "/^[a-z]+$/", 4)
    assert got == exp.result == (1 if kind == "letters" else 0)


def test_config3_as_written_is_a_parse_error(gctx):
    hs = [gctx.trivial(ord("a"))]
    with pytest.raises(F.ParseError):
        gctx.has_match(hs, "/^[a-z0-9]+$/")


def test_config4_the_i_1024(gctx):
    rng = np.random.default_rng(5)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ ", dtype=np.uint8)
    s = bytes(rng.choice(alpha, 1024)).decode()
    s = s.replace("the", "thx").replace("The", "Thx").replace("tHe", "tHx").replace("thE", "thx").replace("THE", "THX")
    s = s.replace("tHE", "tHX").replace("ThE", "ThX").replace("THe", "THx")
    exp0 = ro.has_match(s, "/the/i").result
    got0, st = _config(gctx, s, "/the/i", 5)
    assert got0 == exp0 == 0 and st.ct_ops == 12263
    s1 = s[:700] + "ThE" + s[703:]
    got1, _ = _config(gctx, s1, "/the/i", 6)
    assert got1 == 1


def test_config5_small(gctx):
    pat = "/^a{2,8}(bc|de)+[^xyz]$/"
    for s in ["aaabcdebcf", "aaabcdebcx", "abcf", "aadef"]:
        exp = ro.has_match(s, pat)
        got, st = _config(gctx, s, pat, 7)
        assert got == exp.result, s
        assert (st.ct_ops, st.cache_hits) == (exp.ct_ops, exp.cache_hits)


def test_config5_512_merged(gctx):
    """BASELINE config 5 at its full 512 chars: beyond the reference's
    enumeration (memory), evaluated by the merged engine (AUTO falls back to it)
    on encrypted content; results vs the oracle's position-set simulator."""
    import random
    pat = "/^a{2,8}(bc|de)+[^xyz]$/"
    rng = random.Random(5)
    c = "aaa" + "".join(rng.choice(["bc", "de"]) for _ in range(254)) + "f"
    got, st = _config(gctx, c, pat, 11)  # engine AUTO
    assert got == ro.has_match_reach(c, pat) == 1
    gctx.set_engine(F.ENGINE_MERGED)
    try:
        bad = c[:300] + "x" + c[301:]
        got, st = _config(gctx, bad, pat, 12)
        assert got == ro.has_match_reach(bad, pat) == 0
    finally:
        gctx.set_engine(F.ENGINE_AUTO)


def test_config3_as_written_256(gctx):
    """BASELINE config 3, /^[a-z0-9]+$/ on 256 encrypted chars, under the
    opt-in grammar extension (the reference returns Err): positive content and
    negatives one character outside a range, vs the oracle's extension."""
    import random
    from test_grammar_ext import CONFIG3, config3_contents
    pos, negs = config3_contents(random.Random(3))
    with pytest.raises(F.ParseError):
        _config(gctx, pos[:8], CONFIG3, 13)
    gctx.set_grammar(F.GRAMMAR_EXT)
    try:
        for i, s in enumerate([pos, negs[0], negs[4]]):
            got, st = _config(gctx, s, CONFIG3, 14 + i)
            exp = ro.has_match(s, CONFIG3, ext=True)
            assert got == exp.result == (1 if s == pos else 0), i
            assert (st.ct_ops, st.cache_hits) == (exp.ct_ops, exp.cache_hits)
    finally:
        gctx.set_grammar(F.GRAMMAR_REFERENCE)


def test_faithful_lowering(gctx):
    rng = np.random.default_rng(8)
    s = _printable(rng, 64)
    s = s[:10] + "abc" + s[13:]
    gctx.set_lowering(F.LOWER_FAITHFUL)
    try:
        got, st = _config(gctx, s, "/abc/", 8)
    finally:
        gctx.set_lowering(F.LOWER_THRESHOLD)
    assert got == 1 and st.pbs == 743


def test_start_range_shards_or_to_full(gctx):
    rng = np.random.default_rng(9)
    s = _printable(rng, 96)
    s = s[:60] + "abc" + s[63:]
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=10))
    parts = []
    for lo, hi in [(0, 32), (32, 64), (64, 96)]:
        out, _ = gctx.has_match(hs, "/abc/", lo, hi)
        parts.append(out)
    dec = [gctx.decrypt_radix(gctx.download_radix(p)) for p in parts]
    assert dec == [0, 1, 0]
    assert gctx.decrypt_radix(gctx.download_radix(gctx.or_many(parts))) == 1


def test_plan_cache_replays_bit_identical(gctx):
    """A repeat has_match replays the cached plan: same output ciphertext words,
    same counters, no host lowering; another start range misses."""
    rng = np.random.default_rng(11)
    s = _printable(rng, 48)
    s = s[:30] + "abc" + s[33:]
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=12))
    o1, st1 = gctx.has_match(hs, "/abc/")
    o2, st2 = gctx.has_match(hs, "/abc/")
    assert st2.plan_cached == 1
    assert (st1.ct_ops, st1.pbs, st1.blind_rotations, st1.levels) == (st2.ct_ops, st2.pbs, st2.blind_rotations, st2.levels)
    w1, w2 = gctx.download_radix(o1), gctx.download_radix(o2)
    assert np.array_equal(w1, w2) and gctx.decrypt_radix(w2) == 1
    o3, st3 = gctx.has_match(hs, "/abc/", 0, 20)
    assert st3.plan_cached == 0 and gctx.decrypt_radix(gctx.download_radix(o3)) == 0
    gctx.set_plan_cache(0)
    try:
        o7, st7 = gctx.has_match(hs, "/abc/")
        assert st7.plan_cached == 0 and np.array_equal(gctx.download_radix(o7), w1)
    finally:
        gctx.set_plan_cache(8)
    for h in hs + [o1, o2, o3, o7]:
        gctx.release(h)


@pytest.fixture(scope="module")
def cold_ctx(gctx, key_blob):
    """A second context with the same keys (same server-key seed) and the plan cache
    off: the cold reference a cached plan must match bit for bit."""
    p = gctx.params
    ctx = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    ctx.set_plan_cache(0)
    return ctx


def _cold(gctx, cold, hs, pattern):
    """has_match in the cold context on the same ciphertext words (trivial handles stay
    trivial, a handle used twice maps to one handle): the plan compiled for these very
    slots, no cache involved"""
    mapped, seen = [], {}
    for h in hs:
        if h not in seen:
            w = gctx.download_radix(h)
            if not w[:, :-1].any():  # zero masks: a trivial radix (body m * 2^59 per block)
                seen[h] = cold.trivial(sum(int(w[b, -1] >> np.uint64(59)) << (2 * b) for b in range(4)))
            else:
                seen[h] = cold.upload_radix(w)[0]
        mapped.append(seen[h])
    o, st = cold.has_match(mapped, pattern)
    w = cold.download_radix(o)
    for h in set(seen.values()) | {o}:
        cold.release(h)
    return w, st


def test_plan_cache_fresh_content_hits(gctx, cold_ctx):
    """The plan is keyed on the content's shape, not its slots (engine.rs:8-42
    re-plans every call; the circuit depends only on pattern and length): freshly
    encrypted content of the same length hits the cached plan, and its result is
    bit-identical to a cold plan compiled for that content's own slots."""
    rng = np.random.default_rng(21)
    base = _printable(rng, 40).replace("abc", "abd")
    texts = [base[:12] + "abc" + base[15:], base, base[:33] + "abc" + base[36:]]
    gctx.set_plan_cache(0)
    gctx.set_plan_cache(8)
    first = None
    for i, t in enumerate(texts):
        hs = gctx.upload_radix(gctx.encrypt_str(t, seed=30 + i))
        o, st = gctx.has_match(hs, "/abc/")
        assert st.plan_cached == (0 if first is None else 1), i
        w = gctx.download_radix(o)
        cold, st_c = _cold(gctx, cold_ctx, hs, "/abc/")
        assert np.array_equal(w, cold), i
        assert gctx.decrypt_radix(w) == ro.has_match(t, "/abc/").result
        assert (st.pbs, st.blind_rotations, st.levels) == (st_c.pbs, st_c.blind_rotations, st_c.levels)
        first = first or st
        for h in hs + [o]:
            gctx.release(h)


def test_plan_cache_released_slots_reused(gctx, cold_ctx):
    """Content released and new content uploaded into the same arena slots: the
    cache hit reads the new ciphertexts (the content map is bound per call)."""
    s1, s2 = "zzabczzzz", "zzzzzzzzz"
    hs = gctx.upload_radix(gctx.encrypt_str(s1, seed=40))
    o, _ = gctx.has_match(hs, "/abc/")
    assert gctx.decrypt_radix(gctx.download_radix(o)) == 1
    for h in hs + [o]:
        gctx.release(h)
    hs2 = gctx.upload_radix(gctx.encrypt_str(s2, seed=41))
    o2, st2 = gctx.has_match(hs2, "/abc/")
    assert st2.plan_cached == 1 and gctx.decrypt_radix(gctx.download_radix(o2)) == 0
    assert np.array_equal(gctx.download_radix(o2), _cold(gctx, cold_ctx, hs2, "/abc/")[0])
    for h in hs2 + [o2]:
        gctx.release(h)


def test_plan_cache_content_shape(gctx, cold_ctx):
    """Other shapes miss: a trivial character where the cached plan had a
    ciphertext, and one ciphertext at two positions (merged by the executor);
    each result is bit-identical to its cold plan."""
    t = "xabcabx"
    hs = gctx.upload_radix(gctx.encrypt_str(t, seed=50))
    o, st = gctx.has_match(hs, "/abc/")
    shapes = [[hs[0], gctx.trivial(ord("a"))] + hs[2:],      # trivial block
              hs[:4] + [hs[1], hs[2]] + hs[6:]]                # "xabcabx" with shared handles
    for sh in shapes:
        o2, st2 = gctx.has_match(sh, "/abc/")
        assert st2.plan_cached == 0
        w = gctx.download_radix(o2)
        assert np.array_equal(w, _cold(gctx, cold_ctx, sh, "/abc/")[0])
        assert gctx.decrypt_radix(w) == 1
        o3, st3 = gctx.has_match(sh, "/abc/")
        assert st3.plan_cached == 1 and np.array_equal(gctx.download_radix(o3), w)
        gctx.release(o2)
        gctx.release(o3)
    for h in hs + [o]:
        gctx.release(h)


def test_plan_cache_slot_budget(gctx, cold_ctx):
    """A plan larger than the slot budget runs uncached (same bits); the budget
    evicts before allocating and the held slots never exceed it."""
    hs = gctx.upload_radix(gctx.encrypt_str("qqabcq" * 6, seed=60))
    ref, _ = _cold(gctx, cold_ctx, hs, "/abc/")
    gctx.set_plan_cache_slots(10)
    try:
        o, st = gctx.has_match(hs, "/abc/")
        o2, st2 = gctx.has_match(hs, "/abc/")
        assert st.plan_cached == st2.plan_cached == 0
        assert np.array_equal(gctx.download_radix(o2), ref)
        assert gctx.plan_cache_stats()["slots"] <= 10
    finally:
        gctx.set_plan_cache_slots(1 << 18)
    o3, st3 = gctx.has_match(hs, "/abc/")
    assert st3.plan_cached == 0 and gctx.plan_cache_stats()["slots"] <= 1 << 18
    for h in hs + [o, o2, o3]:
        gctx.release(h)


@pytest.mark.parametrize("pattern", ["/abc/", "/^a{2,8}(bc|de)+[^xyz]$/"])
def test_has_match_batch_bit_identical(gctx, cold_ctx, pattern):
    """fr_has_match_batch: M matches of one pattern in shared launches, each output
    bit-identical to fr_has_match on its own content (cold plan), levels unchanged,
    rotations M times one match's; a repeat with fresh content hits the plan."""
    rng = np.random.default_rng(70)
    if pattern == "/abc/":
        texts = [_printable(rng, 24).replace("abc", "abd") for _ in range(3)]
        texts[1] = texts[1][:5] + "abc" + texts[1][8:]
    else:
        texts = ["aaabcdebcf", "aaabcdebcx", "aadebcbcdf"]
    hss = [gctx.upload_radix(gctx.encrypt_str(t, seed=71 + i)) for i, t in enumerate(texts)]
    outs, st = gctx.has_match_batch(hss, pattern)
    _, st1 = _cold(gctx, cold_ctx, hss[0], pattern)
    assert st.blind_rotations == len(texts) * st1.blind_rotations and st.levels == st1.levels
    for t, hs, o in zip(texts, hss, outs):
        w = gctx.download_radix(o)
        assert np.array_equal(w, _cold(gctx, cold_ctx, hs, pattern)[0]), t
        assert gctx.decrypt_radix(w) == ro.has_match_reach(t, pattern)
        gctx.release(o)
    hss2 = [gctx.upload_radix(gctx.encrypt_str(t, seed=90 + i)) for i, t in enumerate(texts)]
    outs2, st2 = gctx.has_match_batch(hss2[::-1], pattern)
    assert st2.plan_cached == 1
    assert [gctx.decrypt_radix(gctx.download_radix(o)) for o in outs2] == \
        [ro.has_match_reach(t, pattern) for t in texts[::-1]]
    for h in [h for hs in hss + hss2 for h in hs] + outs2:
        gctx.release(h)


def test_async_matches_chain_and_block(gctx):
    """has_match returns once its launches are enqueued (default): the result handle
    feeds further ops at once (NOT, OR), back-to-back matches with released outputs
    reuse slots in stream order, and the blocking mode (fr_set_async 0) gives the same
    words."""
    s1, s2 = "qqabcqqqq", "qqqqqqqqq"
    h1 = gctx.upload_radix(gctx.encrypt_str(s1, seed=80))
    h2 = gctx.upload_radix(gctx.encrypt_str(s2, seed=81))
    outs = []
    for _ in range(3):
        o1, _ = gctx.has_match(h1, "/abc/")
        o2, _ = gctx.has_match(h2, "/abc/")
        n1 = gctx.not_(o1)
        orr = gctx.or_(o1, o2)
        outs.append([gctx.download_radix(x) for x in (o1, o2, n1, orr)])
        for x in (o1, o2, n1, orr):
            gctx.release(x)
    dec = [[gctx.decrypt_radix(w) for w in ws] for ws in outs]
    assert dec == [[1, 0, 0, 1]] * 3
    assert all(np.array_equal(outs[0][i], outs[r][i]) for r in (1, 2) for i in range(2))
    gctx.set_async(False)
    try:
        ob, _ = gctx.has_match(h1, "/abc/")
        assert np.array_equal(gctx.download_radix(ob), outs[0][0])
    finally:
        gctx.set_async(True)
    for h in h1 + h2 + [ob]:
        gctx.release(h)


@pytest.mark.parametrize("level", [1, 2])
def test_profiling_timers(gctx, level):
    """Profiling mode (level 1: bench.py's timed region): per-level BR timers (and at
    level 2 the KS timers) accumulate one launch per level, and the match result is
    unchanged."""
    hs = gctx.upload_radix(gctx.encrypt_str("xxabcxxxxxxxxxxxxxxx", seed=14))
    ref, _ = gctx.has_match(hs, "/abc/")
    t0 = gctx.device_timers()
    gctx.set_profiling(level)
    try:
        out, st = gctx.has_match(hs, "/abc/")
    finally:
        gctx.set_profiling(False)
    t1 = gctx.device_timers()
    assert t1["br_launches"] - t0["br_launches"] == st.levels
    assert t1["br_gates"] - t0["br_gates"] == st.blind_rotations
    assert t1["br_ms"] > t0["br_ms"]
    assert (t1["ks_ms"] > t0["ks_ms"]) == (level == 2)
    assert np.array_equal(gctx.download_radix(out), gctx.download_radix(ref))
    # a blocking call fills the match's own timers; an asynchronous one leaves them 0
    assert st.br_launches == 0 and st.br_kernel_ms == 0.0
    gctx.set_async(False)
    gctx.set_profiling(level)
    try:
        out2, st2 = gctx.has_match(hs, "/abc/")
    finally:
        gctx.set_profiling(False)
        gctx.set_async(True)
    assert st2.br_launches == st2.levels and st2.br_gates == st2.blind_rotations and st2.br_kernel_ms > 0
    assert (st2.ks_kernel_ms > 0) == (level == 2)
    for h in hs + [ref, out, out2]:
        gctx.release(h)


def test_async_match_then_host_hooks(gctx, oracle_k1):
    """An asynchronous has_match still queued when the single-stage test hooks write
    their inputs: both results stay right."""
    O = oracle_k1
    hs = gctx.upload_radix(gctx.encrypt_str("qq" * 60 + "abc" + "q" * 61, seed=15))
    ref, _ = gctx.has_match(hs, "/abc/")
    ref_w = gctx.download_radix(ref)
    ks = O.keyswitch(O.encrypt_blocks([5, 9, 2], seed=16))
    luts = [[(3 * m + j) % 16 for m in range(16)] for j in range(3)]
    for _ in range(2):
        out, _ = gctx.has_match(hs, "/abc/")  # queued, not synchronised
        dev = gctx.dev_blind_rotate(ks, luts)
        for j in range(3):
            assert (dev[j] == O.blind_rotate(ks[j], luts[j])).all(), j
        out2, _ = gctx.has_match(hs, "/abc/")
        mv = gctx.dev_blind_rotate_multi(ks[0], luts[:2])
        assert (mv == O.blind_rotate_multi(ks[0], luts[:2])).all()
        out3, _ = gctx.has_match(hs, "/abc/")
        assert (gctx.dev_keyswitch(O.encrypt_blocks([7], seed=17)) == O.keyswitch(O.encrypt_blocks([7], seed=17))).all()
        for o in (out, out2, out3):
            assert np.array_equal(gctx.download_radix(o), ref_w)
            gctx.release(o)
    for h in hs + [ref]:
        gctx.release(h)


def test_k2_n1024_params_rns(key_blob, fixture_key):
    """The N=1024 variant on the RNS ring (one GGSW per coefficient): the same
    2048-bit key read as k=2 polynomials of 1024."""
    params = F.default_params(k=2, N=1024, ring=F.RING_RNS)
    ctx = F.Context(0, params)
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    O = of.Oracle(fixture_key, seed=SEED, k=2, N=1024, ring=of.RING_RNS)
    ksk, bsk = ctx.export_server_key()
    assert (ksk == O.ksk).all() and (bsk == O.bsk).all()
    blocks = O.encrypt_blocks([6, 1], seed=5)
    ks = O.keyswitch(blocks)
    lut = [(5 * m + 2) % 16 for m in range(16)]
    got = ctx.dev_blind_rotate(ks[:1], [lut])
    assert (got[0] == O.blind_rotate(ks[0], lut)).all()
    got, st = _config(ctx, "xxabcx", "/abc/", 11)
    assert got == 1


def test_rns_ring_smoke(key_blob, fixture_key):
    """The opt-in RNS/NTT ring at the reference parameters: server key equal to the
    oracle's, one blind rotation bit-exact, a small match decrypting right."""
    ctx = F.Context(0, F.default_params(k=1, N=2048, ring=F.RING_RNS))
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    O = of.Oracle(fixture_key, seed=SEED, ring=of.RING_RNS)
    ks = O.keyswitch(O.encrypt_blocks([11], seed=6))
    assert (ctx.dev_keyswitch(O.encrypt_blocks([11], seed=6)) == ks).all()
    lut = [(9 * m + 4) % 16 for m in range(16)]
    assert (ctx.dev_blind_rotate(ks, [lut])[0] == O.blind_rotate(ks[0], lut)).all()
    got, _ = _config(ctx, "qqabcq", "/abc/", 12)
    assert got == 1


def test_fuzz_scale_vs_oracle(gctx):
    """20 seeded random patterns on 64-300 encrypted chars (tests/golden/fuzz_scale.json,
    made by make_fuzz_scale.py from the oracle's position-set simulator): multi-launch
    levels, the throughput shape, circuits of up to ~400 levels and plan-cache
    eviction on random circuits; each decrypted result against the oracle's."""
    cases = load("fuzz_scale.json")["cases"]
    for i, cse in enumerate(cases):
        hs = gctx.encrypt_upload_str(cse["content"], seed=1000 + i)
        out, st = gctx.has_match(hs, cse["pattern"])
        assert gctx.decrypt_radix(gctx.download_radix(out)) == cse["expected"], (i, cse["pattern"])
        for h in hs + [out]:
            gctx.release(h)


@pytest.mark.gpu
def test_c_abi_consumer_gpu(tmp_path):
    """The engine end to end from plain C on device 0 (tests/c_abi_consumer.c ... gpu):
    server key, device encryption, has_match planted and absent, download and decrypt
    under the fixture key, the reference's Err on the device path."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    lib_dir = os.path.join(repo, "fhe-regex_amd")
    exe = str(tmp_path / "c_abi_consumer")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(repo, "include"),
                    os.path.join(here, "c_abi_consumer.c"), "-o", exe, "-L", lib_dir, "-lfheregex",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    res = subprocess.run([exe, os.path.join(here, "golden", "client_key"), "gpu"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert "ok" in res.stdout


def test_fuzz_boundary_vs_oracle(gctx):
    """30 seeded random patterns on 256-512 encrypted chars with a matching string, or a
    one-character near miss of it, planted at the first or the last start offsets
    (tests/golden/fuzz_boundary.json, made by make_fuzz_boundary.py from the oracle's
    position-set simulator; 22 match, 8 do not): start-offset and anchor boundaries
    (engine.rs:15-18, 51-57) on full-size random circuits, each decrypted result against
    the oracle's."""
    cases = load("fuzz_boundary.json")["cases"]
    for i, cse in enumerate(cases):
        hs = gctx.encrypt_upload_str(cse["content"], seed=2000 + i)
        out, st = gctx.has_match(hs, cse["pattern"])
        assert gctx.decrypt_radix(gctx.download_radix(out)) == cse["expected"], (i, cse["pattern"], cse["at"])
        for h in hs + [out]:
            gctx.release(h)


def test_fuzz_encrypted_vs_oracle(gctx):
    """Seeded random patterns (the reference grammar, tests/regex_fuzz.py) on random
    encrypted content of 1-10 chars (engine AUTO), each decrypted result against the
    oracle's position-set simulator (polynomial; the enumerating oracle's counters are
    checked on the host, tests/test_host.py), the reference's Err / panic reproduced;
    the plan cache evicts as it goes."""
    import random

    import regex_fuzz as rf
    rng = random.Random(11)
    n = errs = 0
    while n < 60:
        p = rf.rand_pattern(rng)
        c = rf.rand_content(rng, rng.randint(1, 10))
        try:
            exp = ro.has_match_reach(c, p)
        except (ro.ParseError, ro.ReferencePanic) as e:
            hs = gctx.encrypt_upload_str(c, seed=n)
            with pytest.raises(F.ParseError if isinstance(e, ro.ParseError) else F.ReferencePanic):
                gctx.has_match(hs, p)
            for h in hs:
                gctx.release(h)
            errs += 1
            continue
        hs = gctx.encrypt_upload_str(c, seed=n)
        out, st = gctx.has_match(hs, p)
        assert gctx.decrypt_radix(gctx.download_radix(out)) == exp, (c, p)
        for h in hs + [out]:
            gctx.release(h)
        n += 1


# ------------------------------------------------ whole matches, word for word
def _match_words_vs_oracle(gctx, O, content, pattern, seed, engine=F.ENGINE_AUTO, grammar=F.GRAMMAR_REFERENCE,
                           lowering=F.LOWER_THRESHOLD, multi_value=True):
    """One has_match on the device against the oracle's evaluation of the same lowered
    schedule (fr_schedule_match: fr_job semantics, oracle_ffi.run_schedule) on the same
    content LWEs and the same server key: the result ciphertext word for word
    (execution.rs:64-222 and the fold engine.rs:22-35, through every level's keyswitch
    and blind rotation)."""
    ct = gctx.encrypt_str(content, seed=seed)
    hs = gctx.upload_radix(ct)
    out, st = gctx.has_match(hs, pattern)
    got = gctx.download_radix(out)
    S = F.schedule_match(len(content), pattern, engine=engine, grammar=grammar, lowering=lowering,
                         multi_value=multi_value)
    assert (len(S.jobs), len(S.level_off) - 1) == (st.blind_rotations, st.levels)
    exp = O.run_schedule(S, ct)
    assert np.array_equal(got[0], exp), (pattern, len(content))
    assert not got[1:].any()  # blocks 1..3 of the boolean radix: trivial zeros
    for h in hs + [out]:
        gctx.release(h)
    return int(O.decode16(exp)[0] == 1)


def test_match_words_abc_64(gctx, oracle_k1):
    rng = np.random.default_rng(31)
    s = _printable(rng, 64).replace("abc", "abd")
    assert _match_words_vs_oracle(gctx, oracle_k1, s[:40] + "abc" + s[43:], "/abc/", 32) == 1
    assert _match_words_vs_oracle(gctx, oracle_k1, s, "/abc/", 33) == 0


def test_match_words_range_64(gctx, oracle_k1):
    rng = np.random.default_rng(34)
    s = "".join(chr(c) for c in rng.integers(ord("b"), ord("z") + 1, 64))
    assert _match_words_vs_oracle(gctx, oracle_k1, s, "/^[a-z]+$/", 35) == 1
    assert _match_words_vs_oracle(gctx, oracle_k1, s[:50] + "A" + s[51:], "/^[a-z]+$/", 36) == 0


def test_match_words_config5_small(gctx, oracle_k1):
    pat = "/^a{2,8}(bc|de)+[^xyz]$/"
    for i, s in enumerate(["aaabcdebcf", "aaabcdebcx", "aadef"]):
        assert _match_words_vs_oracle(gctx, oracle_k1, s, pat, 37 + i) == ro.has_match_reach(s, pat), s


@pytest.mark.parametrize("case", [3, 9, 11, 17, 19])
def test_match_words_fuzz_scale(gctx, oracle_k1, case):
    """Five fuzz_scale.json cases of 500-950 rotations (case 9: 204 dependent levels)."""
    cse = load("fuzz_scale.json")["cases"][case]
    assert _match_words_vs_oracle(gctx, oracle_k1, cse["content"], cse["pattern"], 3000 + case) == cse["expected"]


@pytest.mark.parametrize("world", [2, 3])
def test_match_words_start_shards(gctx, oracle_k1, world):
    """north_star's start-offset shards word for word: each rank's fr_has_match_range over
    its start range on its content window against the oracle's evaluation of the same
    ranged schedule (fr_schedule_match with start_lo / start_hi) on the same LWEs, and the
    final bitor (Context.or_each: one sign gate over the ranks' booleans) against the
    oracle's gate.  /the/i on 192 letters with "ThE" planted across the first shard
    boundary (engine.rs:15-35)."""
    L, pat = 192, "/the/i"
    rng = np.random.default_rng(53 + world)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ ", dtype=np.uint8)
    s = bytearray(rng.choice(alpha, L))
    for i in range(L - 2):
        if bytes(s[i:i + 3]).lower() == b"the":
            s[i + 2] = ord("x")
    cut = F.shard_starts(L, world, 1)[0]
    s[cut - 1:cut + 2] = b"ThE"
    s = bytes(s)
    O = oracle_k1
    words, parts, held = [], [], []
    for r in range(world):
        lo, hi = F.shard_starts(L, world, r)
        wlo, whi = F.content_window(L, pat, lo, hi)
        win = gctx.encrypt_str(s[wlo:whi], seed=70 + r)  # [whi - wlo, 4, lwe]
        full = np.zeros((L, 4, gctx.lwe_len), dtype=np.uint64)
        full[wlo:whi] = win
        hs = [F.NULL_CT] * L
        hs[wlo:whi] = gctx.upload_radix(win)
        out, st = gctx.has_match(hs, pat, lo, hi)
        got = gctx.download_radix(out)
        S = F.schedule_match(L, pat, lo, hi)
        assert (len(S.jobs), len(S.level_off) - 1) == (st.blind_rotations, st.levels)
        exp = O.run_schedule(S, full)
        assert np.array_equal(got[0], exp), r
        words.append(exp)
        parts.append(out)
        held += hs[wlo:whi]
    res = gctx.or_each([parts])[0]
    exp_or = O.gates([([(q, 1) for q in range(world)], -1, [0] * 16, 2)], np.stack(words))[0]
    assert np.array_equal(gctx.download_radix(res)[0], exp_or)
    assert O.decode16(exp_or)[0] == 1 == ro.has_match_reach(s.decode(), pat)
    for h in held + parts + [res]:
        gctx.release(h)


@pytest.mark.parametrize("world", [2, 4])
def test_match_parts_words_start_shards(gctx, oracle_k1, world):
    """fr_has_match_parts word for word: each rank's 16 // world parts (its OR tree stopped
    one level early) against the oracle's evaluation of the same parts schedule on the same
    LWEs, then ONE threshold OR over every rank's parts (Context.or_each) against the
    oracle's gate: the unsharded match's level count, and its result.  /the/i on 192
    letters, "ThE" across the first shard boundary."""
    L, pat = 192, "/the/i"
    P = 16 // world
    rng = np.random.default_rng(83 + world)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ ", dtype=np.uint8)
    s = bytearray(rng.choice(alpha, L))
    for i in range(L - 2):
        if bytes(s[i:i + 3]).lower() == b"the":
            s[i + 2] = ord("x")
    cut = F.shard_starts(L, world, 1)[0]
    s[cut - 1:cut + 2] = b"ThE"
    s = bytes(s)
    O = oracle_k1
    words, parts, held = [], [], []
    levels_full = F.schedule_match(L, pat)
    for r in range(world):
        lo, hi = F.shard_starts(L, world, r)
        wlo, whi = F.content_window(L, pat, lo, hi)
        win = gctx.encrypt_str(s[wlo:whi], seed=90 + r)
        full = np.zeros((L, 4, gctx.lwe_len), dtype=np.uint64)
        full[wlo:whi] = win
        hs = [F.NULL_CT] * L
        hs[wlo:whi] = gctx.upload_radix(win)
        outs, st = gctx.has_match_parts(hs, pat, lo, hi, P)
        S = F.schedule_match(L, pat, lo, hi, max_parts=P)
        assert 1 <= len(outs) == len(S.parts) <= P
        assert (len(S.jobs), len(S.level_off) - 1) == (st.blind_rotations, st.levels)
        exp = O.run_schedule_parts(S, full)
        for j, o in enumerate(outs):
            assert np.array_equal(gctx.download_radix(o)[0], exp[j]), (r, j)
        r_exp = int(any(s[i:i + 3].lower() == b"the" for i in range(lo, hi)))
        assert int(any(O.decode16(e)[0] for e in exp)) == r_exp, r
        words += exp
        parts += outs
        held += hs[wlo:whi]
    assert st.levels + 1 == len(levels_full.level_off) - 1  # the last rank's levels + the OR
    res = gctx.or_each([parts])[0]
    exp_or = O.gates([([(q, 1) for q in range(len(parts))], -1, [0] * 16, 2)], np.stack(words))[0]
    assert np.array_equal(gctx.download_radix(res)[0], exp_or)
    assert O.decode16(exp_or)[0] == 1 == ro.has_match_reach(s.decode(), pat)
    for h in held + parts + [res]:
        gctx.release(h)


@pytest.mark.parametrize("case", [3, 11, 17])
def test_match_parts_fuzz_scale(gctx, case):
    """fr_has_match_parts on fuzz_scale.json patterns (500-950 rotations each), the content
    split into three start ranges with 5 parts each: every part decrypts to its plaintext
    value in the host's parts program (fr_plain_match_parts), and each range's OR to the
    range's result"""
    cse = load("fuzz_scale.json")["cases"][case]
    s, pat = cse["content"], cse["pattern"]
    L = len(s)
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=4000 + case))
    got_any = 0
    for r in range(3):
        lo, hi = F.shard_starts(L, 3, r)
        outs, st = gctx.has_match_parts(hs, pat, lo, hi, 5)
        pr, vals = F.plain_match_parts(s, pat, lo, hi, 5, engine=F.ENGINE_AUTO)
        dec = [gctx.decrypt_radix(gctx.download_radix(o)) for o in outs]
        assert dec == vals, (r, dec, vals)
        assert int(any(dec)) == pr.result_recorded
        got_any |= int(any(dec))
        for o in outs:
            gctx.release(o)
    assert got_any == cse["expected"]
    for h in hs:
        gctx.release(h)


def test_match_parts_cached_and_uncached_bit_identical(gctx):
    """fr_has_match_parts from a cached plan (its parts are fresh copies of the plan's gate
    slots) and with the plan cache off (parts copied out before the plan's slots are
    freed): the same words, <= max_parts parts, OR = fr_has_match_range's result"""
    rng = np.random.default_rng(87)
    s = _printable(rng, 96).replace("abc", "abd")
    s = s[:40] + "abc" + s[43:]
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=88))
    runs = []
    for cache in (8, 8, 0):
        gctx.set_plan_cache(cache)
        outs, st = gctx.has_match_parts(hs, "/abc/", 16, 80, 16)
        runs.append(([gctx.download_radix(o) for o in outs], st.plan_cached))
        for o in outs:
            gctx.release(o)
    gctx.set_plan_cache(8)
    assert [c for _, c in runs] == [0, 1, 0]
    w0 = runs[0][0]
    assert 1 < len(w0) <= 16
    for w, _ in runs[1:]:
        assert len(w) == len(w0) and all(np.array_equal(a, b) for a, b in zip(w, w0))
    one, _ = gctx.has_match(hs, "/abc/", 16, 80)
    assert int(any(gctx.decrypt_radix(w) for w in w0)) == gctx.decrypt_radix(gctx.download_radix(one)) == 1
    for h in hs + [one]:
        gctx.release(h)


def test_plan_cache_key_not_forged_by_pattern(gctx):
    """A pattern whose text ends like a cache-key suffix ('|parts4', '|lane1') is a plain
    pattern to the cache: after fr_has_match_parts("/abc/", 4) cached its plan,
    fr_has_match on "/abc/|parts4" still parses (and fails: the reference's Err) instead of
    replaying the parts plan into a one-handle buffer; "/abc|lane\\1/" is its own plan."""
    rng = np.random.default_rng(90)
    s = _printable(rng, 40)
    s = s[:10] + "abc" + s[13:]
    hs = gctx.upload_radix(gctx.encrypt_str(s, seed=91))
    gctx.set_plan_cache(8)
    outs, _ = gctx.has_match_parts(hs, "/abc/", 0, 40, 4)
    assert 1 < len(outs) <= 4
    for bad in ("/abc/|parts4", "/abc/|parts4|lane1"):
        with pytest.raises(F.ParseError):
            gctx.has_match(hs, bad, 0, 40)
    for pat in ("/abc|lane\\1/", "/abc|parts\\4/"):  # valid alternations, checked against the oracle
        o, st = gctx.has_match(hs, pat)
        assert st.plan_cached == 0
        assert gctx.decrypt_radix(gctx.download_radix(o)) == ro.has_match(s, pat).result == 1
        gctx.release(o)
    for h in hs + outs:
        gctx.release(h)


# ------------------------------------- start-offset shards across contexts
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("where", ["boundary", "absent"])
def test_start_shards_two_contexts_config4(gctx, key_blob, world, where):
    """north_star's start-offset shards (engine.rs:15-35) with one context per rank on
    device 0: each context holds only the content window its start range reads
    (F.content_window), runs fr_has_match_range, exports its boolean device to device
    into its row of one buffer (fr_export_bool_device); the first context imports the
    rows (fr_import_bool_device) and ORs them (fr_or_many).  BASELINE config 4
    (/the/i on 1024 chars) with "ThE" across a shard boundary, and absent."""
    import torch
    p = gctx.params
    L, pat = 1024, "/the/i"
    rng = np.random.default_rng(47)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ ", dtype=np.uint8)
    s = bytearray(rng.choice(alpha, L))
    for i in range(L - 2):
        if bytes(s[i:i + 3]).lower() == b"the":
            s[i + 2] = ord("x")
    if where == "boundary":
        cut = F.shard_starts(L, world, 1)[0]  # first start of rank 1: "ThE" starts on rank 0's last start
        s[cut - 1:cut + 2] = b"ThE"
    s = bytes(s)
    exp = ro.has_match_reach(s.decode(), pat)
    assert exp == (1 if where == "boundary" else 0)
    ctxs = [gctx]
    for _ in range(world - 1):
        c = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
        c.load_client_key(key_blob)
        c.gen_server_key(SEED)
        ctxs.append(c)
    buf = torch.zeros((world, gctx.lwe_len), dtype=torch.int64, device="cuda:0")
    held = []
    for r, c in enumerate(ctxs):
        lo, hi = F.shard_starts(L, world, r)
        wlo, whi = F.content_window(L, pat, lo, hi)
        assert lo <= wlo and whi <= min(L, hi + 2)  # /the/ reads at most 2 characters past a start
        hs = [F.NULL_CT] * L
        win = c.upload_radix(c.encrypt_str(s[wlo:whi], seed=60 + r))
        hs[wlo:whi] = win
        out, _ = c.has_match(hs, pat, lo, hi)
        assert c.decrypt_radix(c.download_radix(out)) == int(any(s[i:i + 3].lower() == b"the" for i in range(lo, hi)))
        c.export_bool_device([out], buf[r].data_ptr())
        held.append((c, win + [out]))
    torch.cuda.synchronize()
    parts = gctx.import_bool_device(buf.data_ptr(), world)
    res = gctx.or_many(parts)
    assert gctx.decrypt_radix(gctx.download_radix(res)) == exp
    for c, hs in held:
        for h in hs:
            c.release(h)
    for h in parts + [res]:
        gctx.release(h)
    for c in ctxs[1:]:
        c.close()


def test_export_async_and_or_each(gctx):
    """The bench's start-shard pipeline pieces: a stream-ordered export right after an
    asynchronous match (no synchronisation in between) writes the same words as the
    synchronising export; or_each ORs groups in one launch like or_many."""
    import torch
    hs1 = gctx.upload_radix(gctx.encrypt_str("zzabczzzzz", seed=90))
    hs0 = gctx.upload_radix(gctx.encrypt_str("zzzzzzzzzz", seed=91))
    lib_stream = torch.cuda.ExternalStream(gctx.stream_ptr(), device=torch.device("cuda", 0))
    buf = torch.empty((4, gctx.lwe_len), dtype=torch.int64, device="cuda:0")
    lib_stream.wait_stream(torch.cuda.current_stream())  # the exports run after the allocation's work
    outs = []
    for i, hs in enumerate([hs1, hs0, hs0, hs1]):
        o, _ = gctx.has_match(hs, "/abc/")
        gctx.export_bool_device_async([o], buf[i].data_ptr())
        outs.append(o)
    ev = torch.cuda.Event()
    ev.record(lib_stream)
    ev.synchronize()
    ref = torch.zeros_like(buf)
    gctx.export_bool_device(outs, ref.data_ptr())
    assert torch.equal(buf, ref)
    parts = gctx.import_bool_device(buf.data_ptr(), 4)
    res = gctx.or_each([parts[:2], parts[1:3], parts[2:], [parts[3]]])
    assert [gctx.decrypt_radix(gctx.download_radix(r)) for r in res] == [1, 0, 1, 1]
    assert np.array_equal(gctx.download_radix(res[0]), gctx.download_radix(gctx.or_many(parts[:2])))
    for h in hs1 + hs0 + outs + parts + res:
        gctx.release(h)


@pytest.mark.parametrize("which", ["metric", "config3", "config4", "config5"])
def test_match_words_full_size_configs(gctx, oracle_k1, which):
    """Whole BASELINE workloads at their full sizes, word for word against the oracle's
    evaluation of the same schedule on the same LWEs: /abc/ x 256 (783 rotations), config 3
    as written under the grammar extension (785), config 4 /the/i x 1024 (3,139 rotations, 5
    levels) and config 5 on 512 chars through the merged engine (1,817 rotations, 9 levels)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    pat, kind, L = {"metric": ("/abc/", "printable", 256), "config3": ("/^[a-z0-9]+$/", "alnum", 256),
                    "config4": ("/the/i", "letters", 1024), "config5": (bench.CONFIG5, "config5", 512)}[which]
    content = bench.make_content(kind, L, seed=3).decode()
    grammar = F.GRAMMAR_EXT if which == "config3" else F.GRAMMAR_REFERENCE
    gctx.set_grammar(grammar)
    try:
        got = _match_words_vs_oracle(gctx, oracle_k1, content, pat, 4000 + L, grammar=grammar)
    finally:
        gctx.set_grammar(F.GRAMMAR_REFERENCE)
    exp = ro.has_match_reach(content, pat, ext=True) if which == "config3" else ro.has_match_reach(content, pat)
    assert got == exp == 1


@pytest.mark.parametrize("variant", ["faithful", "faithful_tree", "no-multi-value"])
def test_match_words_lowering_variants(gctx, oracle_k1, variant):
    """The reference-structured lowering (FR_LOWER_FAITHFUL: one gate group per smart_*
    op, execution.rs:64-195; 743 PBS for /abc/ x 64), the same gates with the fold's
    AND/OR chains rebalanced (FR_LOWER_FAITHFUL_TREE: 743 PBS in 10 levels instead of 65)
    and the threshold lowering without multi-value bootstrapping, word for word against
    the oracle's schedule evaluation."""
    rng = np.random.default_rng(41)
    s = _printable(rng, 64).replace("abc", "abd")
    s = s[:20] + "abc" + s[23:]
    mode = {"faithful": F.LOWER_FAITHFUL, "faithful_tree": F.LOWER_FAITHFUL_TREE}.get(variant, F.LOWER_THRESHOLD)
    gctx.set_lowering(mode)
    if variant == "no-multi-value":
        gctx.set_multi_value(False)
    try:
        got = _match_words_vs_oracle(gctx, oracle_k1, s, "/abc/", 42, lowering=mode,
                                     multi_value=variant != "no-multi-value")
    finally:
        gctx.set_lowering(F.LOWER_THRESHOLD)
        gctx.set_multi_value(True)
    assert got == 1


def test_faithful_tree_full_metric(gctx, oracle_k1):
    """FR_LOWER_FAITHFUL_TREE on the metric workload (/abc/ x 256): the reference's 3,047
    PBS in 12 levels, word for word against the oracle's schedule evaluation"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    content = bench.make_content("printable", 256, seed=3).decode()
    gctx.set_lowering(F.LOWER_FAITHFUL_TREE)
    try:
        got = _match_words_vs_oracle(gctx, oracle_k1, content, "/abc/", 4321, lowering=F.LOWER_FAITHFUL_TREE)
        hs = gctx.upload_radix(gctx.encrypt_str(content, seed=4322))
        out, st = gctx.has_match(hs, "/abc/")
        assert gctx.decrypt_radix(gctx.download_radix(out)) == 1
        for h in hs + [out]:
            gctx.release(h)
    finally:
        gctx.set_lowering(F.LOWER_THRESHOLD)
    assert got == 1
    assert (st.pbs, st.levels) == (3047, 12)


def test_lanes_bit_identical(gctx, key_blob):
    """fr_set_lanes: consecutive asynchronous matches round-robin over 3 lanes (streams) of ONE
    context with one key, each lane its own plan copy: every output word for word equal to the
    one-lane match; an OR on lane 0 right after them (device-side join, no host wait) reads
    finished results; released handles and slots are reused across lanes safely"""
    p = gctx.params
    ctx = F.Context(device=0, params=F.default_params(k=p.k, N=p.N, ring=p.ring))
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    rng = np.random.default_rng(61)
    texts = []
    for i in range(3):
        t = _printable(rng, 64).replace("abc", "abd")
        texts.append(t[:10 * i + 5] + "abc" + t[10 * i + 8:] if i != 1 else t)
    hs = [ctx.upload_radix(ctx.encrypt_str(t, seed=80 + i)) for i, t in enumerate(texts)]
    ref = []
    for h in hs:
        o, _ = ctx.has_match(h, "/abc/")
        ref.append(ctx.download_radix(o))
        ctx.release(o)
    exp = [ro.has_match_reach(t, "/abc/") for t in texts]
    assert [ctx.decrypt_radix(w) for w in ref] == exp == [1, 0, 1]
    ctx.set_lanes(3)
    try:
        for rnd in range(2):  # the second round reuses the first round's released slots
            outs = [ctx.has_match(hs[i % 3], "/abc/")[0] for i in range(7)]
            both = ctx.or_many([outs[1], outs[2]])  # lane 0, after the lanes' work
            for i, o in enumerate(outs):
                assert np.array_equal(ctx.download_radix(o), ref[i % 3]), (rnd, i)
            assert ctx.decrypt_radix(ctx.download_radix(both)) == 1
            for o in outs + [both]:
                ctx.release(o)
        # batched and ranged matches go to the lanes too (their own plans), still exact
        bo, _ = ctx.has_match_batch([hs[0], hs[2]], "/abc/")
        ro_, _ = ctx.has_match(hs[2], "/abc/", 0, 40)
        assert [np.array_equal(ctx.download_radix(b), ref[i]) for b, i in zip(bo, (0, 2))] == [True, True]
        assert ctx.decrypt_radix(ctx.download_radix(ro_)) == int("abc" in texts[2][:42])
        for h in list(bo) + [ro_]:
            ctx.release(h)
    finally:
        ctx.set_lanes(1)
    o, _ = ctx.has_match(hs[0], "/abc/")
    assert np.array_equal(ctx.download_radix(o), ref[0])
    ctx.close()


@pytest.mark.parametrize("case,words", [(3, True), (11, True), (17, True), (8, False), (14, False), (19, False)])
def test_faithful_tree_fuzz_scale(gctx, oracle_k1, case, words):
    """FR_LOWER_FAITHFUL_TREE on fuzz_scale.json patterns (914-4,857 rotations, 11-19 levels
    where the serial fold takes 133-764): word for word against the oracle's evaluation of the
    same schedule (the smaller ones), else the decrypted bit against the position-set simulator"""
    cse = load("fuzz_scale.json")["cases"][case]
    gctx.set_lowering(F.LOWER_FAITHFUL_TREE)
    try:
        if words:
            got = _match_words_vs_oracle(gctx, oracle_k1, cse["content"], cse["pattern"], 5000 + case,
                                         lowering=F.LOWER_FAITHFUL_TREE)
        else:
            hs = gctx.upload_radix(gctx.encrypt_str(cse["content"], seed=5000 + case))
            out, _ = gctx.has_match(hs, cse["pattern"])
            got = gctx.decrypt_radix(gctx.download_radix(out))
            for h in hs + [out]:
                gctx.release(h)
    finally:
        gctx.set_lowering(F.LOWER_THRESHOLD)
    assert got == cse["expected"]
