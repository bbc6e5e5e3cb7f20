"""Packed results on host-only contexts: the packing key, the packing keyswitch's host
restatement, the wire blobs, and the match-starts front end.

The packing key has 3 kN rows; row 3 i + l is a GLWE encryption, under the big key read as k
polynomials, of the constant polynomial s_big[i] 2^(64 - 7 (l + 1)) (include/fheregex.h).
pack_lwes is the plain-loop packing keyswitch the device must reproduce word for word
(tests/test_packed_results_gpu.py); here it is pinned by its algebra and by decryption, and
tests/test_pack_oracle.py holds it word for word to oracle/pack_oracle.py, which shares no code
with it.

The phase-error bound is derived, not tuned: rounding a mask coefficient to 21 bits leaves a
uniform error of std 2^43 / sqrt(3), summed over the ~kN/2 set key bits: sqrt(kN/2) 2^43 /
sqrt(3) ~ 2^47.2; the key's own noise through |digit| <= 64 adds 2^43 at most.  The test asks
for std < sqrt(sigma_in^2 + (2^47.5)^2) with sigma_in the inputs' measured phase error.
"""
import json
import os
import random
import struct

import numpy as np
import pytest

import fheregex as F
import regex_fuzz as rf
import regex_oracle as ro
from test_keyed_rng import stream_u64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POINTS = [(1, 2048), (2, 1024)]
PSEED = 0x9AC4
STREAM_PKSK_MASK = 9
DELTA_LOG = 59


def host(point, key_blob=None):
    k, N = point
    ctx = F.Context(device=-1, params=F.default_params(k=k, N=N))
    if key_blob is not None:
        if k == 1:
            ctx.load_client_key(key_blob)
        else:
            ctx.gen_client_key(7)
    return ctx


def s_big(ctx):
    """the big key's bits from the bincode client key: u64 length, then the words"""
    blob = ctx.serialize_client_key()
    (n,) = struct.unpack_from("<Q", blob, 0)
    return np.frombuffer(blob, dtype="<u8", count=n, offset=8).astype(np.int64)


@pytest.fixture(scope="module")
def keyed(key_blob):
    """default point: a client context holding the full host-generated packing key (~1 s)"""
    ctx = host(POINTS[0], key_blob)
    ctx.gen_packing_key(PSEED)
    return ctx


def signed(x):
    return np.asarray(x, dtype=np.uint64).astype(np.int64)


def negacyclic_phase(ct, s, k, N):
    """B - sum_j A_j S_j over Z_2^64[X] / (X^N + 1), restated without the library: each A_j in
    four 16-bit limbs, exact int64 linear convolutions with the key bits (every sum below
    2^16 N), recombined mod 2^64, and the upper half folded back with a minus sign"""
    ct = np.asarray(ct, dtype=np.uint64)
    acc = np.zeros(N, dtype=np.uint64)
    for j in range(k):
        a, sj = ct[j * N:(j + 1) * N], np.asarray(s[j * N:(j + 1) * N], dtype=np.int64)
        for limb in range(4):
            part = ((a >> np.uint64(16 * limb)) & np.uint64(0xFFFF)).astype(np.int64)
            c = np.convolve(part, sj).astype(np.uint64)  # 2N - 1 coefficients
            c = np.append(c, np.uint64(0))
            acc += (c[:N] - c[N:]) << np.uint64(16 * limb)
    return ct[k * N:] - acc


# ------------------------------------------------------------------ the keyswitch
@pytest.mark.parametrize("n", [1, 2, 2048])
def test_linear_and_exact(keyed, n):
    """trivial LWEs (zero mask) have zero digits: the mask stays zero and the body is
    sum_j b_j X^j word for word, whatever the key"""
    rng = np.random.default_rng(n)
    lwes = np.zeros((n, keyed.lwe_len), dtype=np.uint64)
    lwes[:, -1] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    out = keyed.pack_lwes(lwes)
    N = keyed.params.N
    assert not out[:N].any()
    assert np.array_equal(out[N:N + n], lwes[:, -1]) and not out[N + n:].any()


@pytest.mark.parametrize("n", [1, 33, 2048])
def test_decrypt_and_phase_error(keyed, n):
    rng = np.random.default_rng(100 + n)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    lwes = keyed.encrypt_blocks(bits, seed=77).reshape(n, -1)
    words = keyed.pack_lwes(lwes)
    blob = b"FRPKRES1" + struct.pack("<iiQ", 1, 2048, n) + words.tobytes()
    assert keyed.decrypt_packed(blob) == list(bits)
    # the error the packing adds to the used coefficients, against the derived bound
    s = s_big(keyed)
    want = bits.astype(np.int64) << DELTA_LOG
    e_in = signed(lwes[:, -1] - (lwes[:, :-1] * s.astype(np.uint64)).sum(axis=1, dtype=np.uint64)) - want
    assert np.array_equal(keyed.packed_phase(words), negacyclic_phase(words, s, 1, 2048))
    e_out = signed(keyed.packed_phase(words))[:n] - want
    sigma_in = float(np.sqrt(np.mean(e_in.astype(np.float64) ** 2)))
    sigma_out = float(np.sqrt(np.mean(e_out.astype(np.float64) ** 2)))
    bound = np.sqrt(sigma_in ** 2 + (2.0 ** 47.5) ** 2)
    print(f"n={n}: sigma_in 2^{np.log2(sigma_in):.2f}, sigma_out 2^{np.log2(sigma_out):.2f}, bound 2^{np.log2(bound):.2f}")
    assert np.abs(e_out).max() < 2 ** 52  # 6 bits under the decision threshold 2^58
    assert sigma_out < bound  # (n = 1: the one sample's own magnitude)
    # coefficients past n carry the key's noise only
    assert np.abs(signed(keyed.packed_phase(words))[n:]).max(initial=0) < 2 ** 52


def test_affine_and_constant_inputs(keyed):
    """1 - x packs to the negated bit, a constant to itself, its LWE unread"""
    bits = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    lwes = keyed.encrypt_blocks(bits, seed=5).reshape(5, -1)
    w = [1, -1, -1, 0, 0]
    off = [0, 2, 2, 2, 0]  # units of Delta / 2
    words = keyed.pack_lwes(lwes, w, off)
    blob = b"FRPKRES1" + struct.pack("<iiQ", 1, 2048, 5) + words.tobytes()
    assert keyed.decrypt_packed(blob) == [1, 1, 0, 1, 0]
    # constants alone need no LWEs at all, and leave the mask zero
    only = keyed.pack_lwes(None, [0, 0, 0], [2, 0, 2], n=3)
    assert not only[:2048].any() and list(only[2048:2051] >> np.uint64(DELTA_LOG)) == [1, 0, 1]
    # a trivial boolean handle is such a constant (the only handle a host-only context has)
    one = keyed.not_(keyed.or_many([]))
    assert np.array_equal(keyed.pack_bools_words([one, keyed.or_many([]), one]), only)
    assert keyed.decrypt_packed(keyed.pack_bools([one])) == [1]
    with pytest.raises(F.FheRegexError) as e:
        keyed.pack_bools_words([keyed.trivial(5)])  # a radix handle
    assert e.value.code == F.ERR_INVALID


# ------------------------------------------------------------------ the key
@pytest.mark.parametrize("point", POINTS, ids=["k1n2048", "k2n1024"])
def test_packing_key_rows(point, key_blob):
    k, N = point
    ctx = host(point, key_blob)
    s = s_big(ctx)
    KD = 3 * k * N
    sigma = ctx.params.glwe_sigma * 2.0 ** 64
    key = F.seed_key(PSEED)
    for r in sorted({0, 1, 2, 3 * N - 1, (3 * N) % KD, KD - 1}):
        row = ctx.gen_packing_rows(PSEED, r, r + 1)[0]
        # masks: polynomial j is u64 numbers (r k + j) N + t of STREAM_PKSK_MASK (RFC 8439 ChaCha20)
        assert np.array_equal(row[:k * N], stream_u64(key, STREAM_PKSK_MASK, r * k * N, k * N)), r
        # phase: s_big[i] 2^(64 - 7 (l + 1)) on coefficient 0, nothing elsewhere, within 6 sigma
        ph = ctx.packed_phase(row)
        # (the library's phase shares its rotation helper with the generator: restated in numpy)
        assert np.array_equal(ph, negacyclic_phase(row, s, k, N)), r
        i, l = divmod(r, 3)
        ph[:1] -= np.uint64(int(s[i]) << (64 - 7 * (l + 1)))
        ph = signed(ph)
        assert np.abs(ph).max() < 6 * sigma, (r, int(np.abs(ph).max()))
        assert np.abs(ph).max() > 0
    # a range is its rows
    two = ctx.gen_packing_rows(PSEED, 1, 3)
    assert np.array_equal(two[1], ctx.gen_packing_rows(PSEED, 2, 3)[0])
    # OS-keyed generations share no word
    a, b = ctx.gen_packing_rows(None, 0, 2), ctx.gen_packing_rows(None, 0, 2)
    assert not (a == b).any()


# ------------------------------------------------------------------ the wire
def test_wire(keyed, key_blob):
    blob = keyed.export_packing_key()
    p = keyed.params
    assert len(blob) == keyed.packing_key_size() == 48 + 8 * 6144 * 4096
    assert bytes(blob[:8]) == b"FRPKKEY1"
    assert struct.unpack("<10i", bytes(blob[8:48])) == (p.k, p.N, p.n, p.ks_base_log, p.ks_level, p.pbs_base_log,
                                                         p.pbs_level, F.RING_FFT, 7, 3)
    rows = np.frombuffer(blob, dtype="<u8", offset=48).reshape(6144, 4096)
    assert np.array_equal(rows[6143], keyed.gen_packing_rows(PSEED, 6143, 6144)[0])
    lwes = keyed.encrypt_blocks([1, 0, 1], seed=9).reshape(3, -1)
    want = keyed.pack_lwes(lwes)

    server = host(POINTS[0])  # no client key
    with pytest.raises(F.FheRegexError) as e:  # packing without a key
        server.pack_lwes(lwes)
    assert e.value.code == F.ERR_INVALID and "packing key" in str(e.value)
    with pytest.raises(F.FheRegexError) as e:
        server.pack_bools([server.or_many([])])
    assert e.value.code == F.ERR_INVALID
    with pytest.raises(F.FheRegexError):
        server.export_packing_key()
    server.load_packing_key(blob)
    assert np.array_equal(server.pack_lwes(lwes), want)
    assert np.array_equal(server.export_packing_key(), blob)
    # refused loads leave the installed key working
    def refused(bad):
        with pytest.raises(F.FheRegexError) as e:
            server.load_packing_key(bad)
        assert e.value.code == F.ERR_INVALID
    refused(blob[:-8])
    refused(blob[:47])
    for at, v in ((7, ord("2")), (13, 4), (40, 8), (44, 5)):  # magic, N, the gadget's base and levels
        keep, blob[at] = blob[at], v
        refused(blob)
        blob[at] = keep
    other = host(POINTS[1])
    with pytest.raises(F.FheRegexError) as e:  # the other point's parameters, whatever the length
        other.load_packing_key(blob)
    assert e.value.code == F.ERR_INVALID
    small = np.concatenate([blob[:48], blob[48:48 + 8 * 6144 * 3072]])
    with pytest.raises(F.FheRegexError) as e:  # ... also at the other point's own length
        other.load_packing_key(small)
    assert e.value.code == F.ERR_INVALID and "parameters" in str(e.value)
    assert np.array_equal(server.pack_lwes(lwes), want)

    # result blobs
    res = b"FRPKRES1" + struct.pack("<iiQ", 1, 2048, 3) + want.tobytes()
    assert len(res) == keyed.packed_result_size(3) == 24 + 32768
    assert keyed.decrypt_packed(res) == [1, 0, 1]
    for bad in (res[:-1], res + b"\0", b"FRPKRES2" + res[8:], res[:8] + struct.pack("<ii", 2, 1024) + res[16:],
                res[:16] + struct.pack("<Q", 2049) + res[24:], res[:16] + struct.pack("<Q", 0) + res[24:]):
        with pytest.raises(F.FheRegexError) as e:
            keyed.decrypt_packed(bad)
        assert e.value.code == F.ERR_INVALID
    # a coefficient past n that holds a bit is reported
    with pytest.raises(F.FheRegexError) as e:
        keyed.decrypt_packed(res[:16] + struct.pack("<Q", 2) + res[24:])
    assert e.value.code == F.ERR_INVALID and "past n" in str(e.value)
    with pytest.raises(F.FheRegexError) as e:
        server.decrypt_packed(res)  # no client key
    assert e.value.code == F.ERR_NO_KEY
    for n in (0, 2049):
        with pytest.raises(F.FheRegexError):
            keyed.packed_result_size(n)


def test_empty_reply_has_no_starts(keyed):
    """ServerKey.match_starts of an empty content is a count of 0 chunks"""
    assert F.ClientKey(keyed).decrypt_starts(struct.pack("<I", 0)) == []
    for bad in (b"", struct.pack("<I", 0) + b"x"):
        with pytest.raises(ValueError):
            F.ClientKey(keyed).decrypt_starts(bad)
    with pytest.raises(F.FheRegexError):  # a chunk that is no packed result blob
        F.ClientKey(keyed).decrypt_starts(struct.pack("<I", 1))


def test_server_key_files(keyed, tmp_path):
    """ServerKey.save / load carry the packing key as an optional second file"""
    keyed.gen_server_key(3)
    sk = F.ServerKey(keyed)
    a, b = str(tmp_path / "sk.npz"), str(tmp_path / "pk.bin")
    sk.save(a, packing_path=b)
    assert os.path.getsize(b) == keyed.packing_key_size()
    back = F.ServerKey.load(a, device=-1, packing_path=b)
    assert np.array_equal(back.ctx.export_packing_key(), keyed.export_packing_key())
    plain = F.ServerKey.load(a, device=-1)  # the first file alone is what it was
    with pytest.raises(F.FheRegexError):
        plain.ctx.export_packing_key()


# ------------------------------------------------------------------ match starts
def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        d = json.load(f)
    return d["cases"] if isinstance(d, dict) else d


def start_cases():
    cases = [(v["content"], v["pattern"]) for v in load("engine_vectors.json")]
    cases += [(v["content"], v["pattern"]) for v in load("readme_vectors.json")]
    cases += [("xaybcdbc", "/a|bc|d/"), ("abcabc", "/^abc/"), ("abcabc", "/abc$/"), ("ab", "/^ab$/"), ("", "/a/")]
    rng = random.Random(20251)
    fuzz = 0
    while fuzz < 30:
        p = rf.rand_pattern(rng)
        # the oracle enumerates every variant of a repetition: those patterns get short contents
        c = rf.rand_content(rng, rng.randint(1, 10 if any(ch in p for ch in "*+{?") else 24))
        try:
            ro.parse(p)
        except (ro.ParseError, ro.ReferencePanic):
            continue
        cases.append((c, p))
        fuzz += 1
    return cases


@pytest.mark.parametrize("content,pattern", start_cases(), ids=lambda v: repr(v)[:24])
def test_plain_match_starts(content, pattern):
    L = len(content)
    try:
        want = [ro.has_match(content, pattern, s, s + 1).result for s in range(L)]
    except (ro.ParseError, ro.ReferencePanic) as e:
        with pytest.raises(F.ParseError if isinstance(e, ro.ParseError) else F.ReferencePanic):
            F.plain_match_starts(content, pattern)
        return
    r, low, rec = F.plain_match_starts(content, pattern)
    assert low == want and rec == want
    whole = F.plain_match(content, pattern)
    assert r.result_lowered == r.result_recorded == int(any(want)) == whole.result_lowered
    # a sub-range is the slice
    if L >= 3:
        _, low2, _ = F.plain_match_starts(content, pattern, 1, L - 1)
        assert low2 == want[1:L - 1]


def test_constant_outputs_and_dedupe():
    # an anchored pattern: start 0 is a gate, every other start the constant 0
    S = F.schedule_match_starts(8, "/^abc/")
    assert S.parts[0][0] >= 0 and all(g == -1 and c == 0 for g, _, c in S.parts[1:])
    assert len(S.parts) == 8
    # /abc/ over 16 characters: the merged program's level-1 gates (the nibble tests) are
    # shared by the starts: no more than the ordinary match's
    def level1(s):
        return sum(j.n_out for j in s.jobs[s.level_off[0]:s.level_off[1]])
    starts, whole = F.schedule_match_starts(16, "/abc/"), F.schedule_match(16, "/abc/")
    assert level1(starts) <= level1(whole)
    assert len(starts.parts) == 16
    # the last two starts cannot fit the pattern: constants
    assert [g for g, _, _ in starts.parts[14:]] == [-1, -1]
