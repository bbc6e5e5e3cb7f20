"""The compact (seeded) server key on host-only contexts, both FFT points.

A compact key is a full server key whose mask words are all ChaCha20 words of a public
mask key M = words 0..7 of chacha_block(K, stream 8, 0); its noise is the standard
generator's under the secret K; the gadget of rows r < k sits in the body as -m g S_r
(include/fheregex.h).  On the wire: "FRCSKEY1", eight int32, M, the bodies.

Pins:
- sizes and header of the blob; client -> blob -> keyless server -> both exports;
- the masks are M's streams, pinned through the oracle-pinned standard generator run under
  M; the only difference is the gadget word, by exactly g;
- the noise is K's streams: the residual (phase minus message polynomial) equals the
  standard key's under K word for word and stays below 8 sigma 2^64;
- reproducible under a key or seed, fresh under the OS CSPRNG;
- every malformed blob is refused with ERR_INVALID and leaves the installed key alone.

The residual of a row is phase - message polynomial with phase = B - sum_j A_j S_j over
the exported masks and message polynomial -m g S_r (r < k) or +m g (r = k, coefficient 0)
in both forms: the standard form holds the same phase, its gadget word being part of A_r.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import fheregex as F

K = bytes((37 * i + 11) & 0xFF for i in range(32))  # a fixed 256-bit generator key
SEED = 0x5EED0C0FFEE
POINTS = [(1, 2048), (2, 1024)]
SIZES = {(1, 2048): 36_552_776, (2, 1024): 27_435_080}
U = np.uint64


class Keys:
    """everything derived once per point and shared (read-only) by the tests"""

    def __init__(self, point, key_blob):
        k, N = point
        self.k, self.N = k, N
        self.p = F.default_params(k=k, N=N)
        self.client = self.ctx(key_blob)
        self.client.gen_server_key(K, compact=True)
        self.blob = self.client.export_server_key_compact()
        self.ksk, self.bsk = self.client.export_server_key()
        self.key_blob = key_blob

    def ctx(self, key_blob=None, params=None):
        c = F.Context(device=-1, params=params if params is not None else self.p)
        if key_blob is not None:
            c.load_client_key(key_blob)
        return c

    def standard(self, key):
        c = self.ctx(self.key_blob)
        c.gen_server_key(key)
        return c.export_server_key()


@pytest.fixture(scope="module", params=POINTS, ids=["k1n2048", "k2n1024"])
def keys(request, key_blob):
    return Keys(request.param, key_blob)


def ggsw_messages(s_small):
    """m_w of GGSW w = 3t + g: s_2t s_2t+1, s_2t (1 - s_2t+1), (1 - s_2t) s_2t+1"""
    s = np.asarray(s_small, dtype=np.int64)
    if len(s) % 2:
        s = np.append(s, 0)
    si, sj = s[0::2], s[1::2]
    return np.stack([si & sj, si & (1 - sj), (1 - si) & sj], axis=1).reshape(-1)


def views(keys, ksk, bsk):
    p = keys.p
    W = 3 * ((p.n + 1) // 2)
    return ksk.reshape(-1, p.n + 1), bsk.reshape(W, p.k + 1, p.k + 1, p.N)


def test_sizes_and_header(keys):
    p = keys.p
    W = 3 * ((p.n + 1) // 2)
    want = 72 + 8 * (p.k * p.N * p.ks_level + W * (p.k + 1) * p.N)
    assert want == SIZES[(keys.k, keys.N)]
    assert keys.client.server_key_compact_size() == want
    # the export writes exactly that many bytes (a larger buffer keeps its tail)
    buf = C.create_string_buffer(b"\xA5" * (want + 16), want + 16)
    n = C.c_size_t()
    F._check(F.lib().fr_export_server_key_compact(keys.client.h, buf, want + 16, C.byref(n)))
    assert n.value == want and buf.raw[want:] == b"\xA5" * 16 and buf.raw[:want] == keys.blob
    F._check(F.lib().fr_export_server_key_compact(keys.client.h, None, 0, C.byref(n)))  # size query
    assert n.value == want
    assert F.lib().fr_export_server_key_compact(keys.client.h, buf, want - 1, C.byref(n)) == F.ERR_INVALID
    assert len(keys.blob) == want and keys.blob[:8] == b"FRCSKEY1"
    assert struct.unpack("<8i", keys.blob[8:40]) == (p.k, p.N, p.n, p.ks_base_log, p.ks_level, p.pbs_base_log,
                                                      p.pbs_level, F.RING_FFT)
    assert F.compact_mask_key(keys.blob) == keys.blob[40:72]
    # the bodies are the full key's body words, in order
    kv, bv = views(keys, keys.ksk, keys.bsk)
    body = np.frombuffer(keys.blob, dtype="<u8", offset=72)
    assert np.array_equal(body[:kv.shape[0]], kv[:, p.n])
    assert np.array_equal(body[kv.shape[0]:], bv[:, :, p.k, :].reshape(-1))
    with pytest.raises(ValueError):
        F.compact_mask_key(b"FRCSKEY0" + keys.blob[8:80])


def test_roundtrip_server_without_client_key(keys, tmp_path):
    server = keys.ctx()
    server.load_server_key_compact(keys.blob)
    k2, b2 = server.export_server_key()
    assert np.array_equal(k2, keys.ksk) and np.array_equal(b2, keys.bsk)
    assert server.export_server_key_compact() == keys.blob
    with pytest.raises(F.FheRegexError):
        server.serialize_client_key()  # the server never saw a client key
    # the expanded export is an ordinary server key
    plain = keys.ctx()
    plain.load_server_key(k2, b2)
    k3, b3 = plain.export_server_key()
    assert np.array_equal(k3, keys.ksk) and np.array_equal(b3, keys.bsk)
    # the raw blob through a file
    path = str(tmp_path / "sk.blob")
    F.ServerKey(keys.client).save_compact(path)
    with open(path, "rb") as f:
        assert f.read() == keys.blob
    sk = F.ServerKey.load_compact(path, device=-1, params=keys.p)
    k4, b4 = sk.ctx.export_server_key()
    assert np.array_equal(k4, keys.ksk) and np.array_equal(b4, keys.bsk)
    assert sk.ctx.export_server_key_compact() == keys.blob


def test_masks_are_the_mask_keys_streams(keys, fixture_key):
    p = keys.p
    M = F.compact_mask_key(keys.blob)
    assert M != K and len(M) == 32
    sk, sb = keys.standard(M)  # the oracle-pinned generator, run under the public mask key
    ck, cb = views(keys, keys.ksk, keys.bsk)
    sk, sb = views(keys, sk, sb)
    assert np.array_equal(ck[:, :p.n], sk[:, :p.n])
    m = ggsw_messages(fixture_key["s_small"])
    assert len(m) == cb.shape[0] and 0 < m.sum() < len(m)
    g = U(1) << U(64 - p.pbs_base_log)
    want = np.zeros(cb[:, :, :p.k, :].shape, dtype=U)
    for r in range(p.k):
        want[:, r, r, 0] = m.astype(U) * g
    assert np.array_equal(sb[:, :, :p.k, :] - cb[:, :, :p.k, :], want)


def negacyclic_by_bits(A, S):
    """rows of A (R, N) u64 times the binary polynomial S mod X^N + 1, mod 2^64"""
    N = A.shape[1]
    acc = np.zeros_like(A)
    for u in np.flatnonzero(S):
        u = int(u)
        if u == 0:
            acc += A
        else:
            acc[:, u:] += A[:, :N - u]
            acc[:, :u] -= A[:, N - u:]
    return acc


def sample_ggsws(m, pairs):
    """GGSWs of the first, middle and last coefficient pair (all three g); neighbouring pairs
    where those hold no m = 1"""
    for d in range(pairs // 2):
        ts = sorted({d, pairs // 2 + d, pairs - 1 - d})
        ws = np.array([3 * t + g for t in ts for g in range(3)])
        if set(m[ws]) == {0, 1}:
            return ws
    raise AssertionError("no sample with both messages")


def ksk_residual(p, key, ksk):
    kv = ksk.reshape(-1, p.n + 1)
    rows = kv.shape[0]
    s_small = np.asarray(key["s_small"], dtype=U)
    s_big = np.asarray(key["s_big"], dtype=U)
    dot = kv[:, :p.n][:, s_small == 1].sum(axis=1, dtype=U)
    i, j = np.arange(rows) // p.ks_level, np.arange(rows) % p.ks_level
    shift = (64 - p.ks_base_log * (j + 1)).astype(U)
    return kv[:, p.n] - dot - (s_big[i] << shift)


def bsk_residual(p, key, bsk, ws, m):
    W = 3 * ((p.n + 1) // 2)
    bv = bsk.reshape(W, p.k + 1, p.k + 1, p.N)[ws]  # (|ws|, k+1 rows, k+1 components, N)
    S = np.asarray(key["s_big"], dtype=U).reshape(p.k, p.N)
    g = U(1) << U(64 - p.pbs_base_log)
    res = bv[:, :, p.k, :].copy()
    for j in range(p.k):
        res -= negacyclic_by_bits(bv[:, :, j, :].reshape(-1, p.N), S[j]).reshape(res.shape)
    mg = m[ws].astype(U) * g
    for r in range(p.k):
        res[:, r, :] += mg[:, None] * S[r][None, :]  # message polynomial -m g S_r
    res[:, p.k, 0] -= mg                              # message polynomial +m g
    return res


def test_noise_is_the_secret_keys_streams(keys, fixture_key):
    p = keys.p
    std2 = keys.standard(K)
    m = ggsw_messages(fixture_key["s_small"])
    ws = sample_ggsws(m, (p.n + 1) // 2)
    assert set(m[ws]) == {0, 1} and len(ws) == 9
    rk_c, rk_s = ksk_residual(p, fixture_key, keys.ksk), ksk_residual(p, fixture_key, std2[0])
    assert len(rk_c) == 10240
    assert np.array_equal(rk_c, rk_s)
    rb_c, rb_s = bsk_residual(p, fixture_key, keys.bsk, ws, m), bsk_residual(p, fixture_key, std2[1], ws, m)
    assert np.array_equal(rb_c, rb_s)
    # 8 sigma: P(|z| > 8) = 1.2e-15 a sample, 10,240 + 9 (k+1) N samples: a tail below 1e-10
    assert np.abs(rk_c.view(np.int64)).max() <= 8 * p.lwe_sigma * 2.0 ** 64
    assert np.abs(rb_c.view(np.int64)).max() <= 8 * p.glwe_sigma * 2.0 ** 64
    assert np.abs(rk_c.view(np.int64)).max() > 0 and np.abs(rb_c.view(np.int64)).max() > 0


def test_fresh_and_reproducible(keys):
    again = keys.ctx(keys.key_blob)
    again.gen_server_key(K, compact=True)
    assert again.export_server_key_compact() == keys.blob
    rows = keys.p.k * keys.p.N * keys.p.ks_level
    a, b = keys.ctx(keys.key_blob), keys.ctx(keys.key_blob)
    a.gen_server_key(None, compact=True)
    b.gen_server_key(None, compact=True)
    ba, bb = a.export_server_key_compact(), b.export_server_key_compact()
    assert F.compact_mask_key(ba) != F.compact_mask_key(bb)
    ka, kb = (np.frombuffer(x, dtype="<u8", offset=72, count=rows) for x in (ba, bb))
    assert (ka != kb).all()
    a.gen_server_key(SEED, compact=True)
    b.gen_server_key(F.seed_key(SEED), compact=True)
    assert a.export_server_key_compact() == b.export_server_key_compact()


def refused(ctx, blob):
    with pytest.raises(F.FheRegexError) as e:
        ctx.load_server_key_compact(blob)
    assert e.value.code == F.ERR_INVALID


def test_refusals_keep_the_installed_key(keys):
    server = keys.ctx()
    server.load_server_key_compact(keys.blob)

    def unchanged():
        assert server.export_server_key_compact() == keys.blob

    bad = [keys.blob[:-1], keys.blob + bytes(8), b"FRCSKEY2" + keys.blob[8:], b"frcskey1" + keys.blob[8:]]
    for i in range(8):  # each header integer in turn
        v = struct.unpack_from("<i", keys.blob, 8 + 4 * i)[0]
        bad.append(keys.blob[:8 + 4 * i] + struct.pack("<i", v + 1) + keys.blob[12 + 4 * i:])
    for b in bad:
        refused(server, b)
        unchanged()
    k2, b2 = server.export_server_key()
    assert np.array_equal(k2, keys.ksk) and np.array_equal(b2, keys.bsk)
    # the other point's blob
    ok, oN = POINTS[1] if (keys.k, keys.N) == POINTS[0] else POINTS[0]
    other = F.Context(device=-1, params=F.default_params(k=ok, N=oN))
    other.load_client_key(keys.key_blob)
    other.gen_server_key(K, compact=True)
    refused(server, other.export_server_key_compact())
    unchanged()
    # the RNS ring has no compact form: generate and load both refuse
    rns = keys.ctx(keys.key_blob, params=F.default_params(k=keys.k, N=keys.N, ring=F.RING_RNS))
    for seed in (SEED, K, None):
        with pytest.raises(F.FheRegexError) as e:
            rns.gen_server_key(seed, compact=True)
        assert e.value.code == F.ERR_INVALID
    refused(rns, keys.blob)
    refused(rns, keys.blob[:36] + struct.pack("<i", F.RING_RNS) + keys.blob[40:])
    with pytest.raises(F.FheRegexError) as e:
        rns.server_key_compact_size()
    assert e.value.code == F.ERR_INVALID
    # no key, a standard-form key, a key installed by fr_load_server_key: no compact export
    empty = keys.ctx(keys.key_blob)
    with pytest.raises(F.FheRegexError) as e:
        empty.export_server_key_compact()
    assert e.value.code == F.ERR_NO_KEY
    with pytest.raises(F.FheRegexError) as e:
        keys.ctx().gen_server_key(K, compact=True)
    assert e.value.code == F.ERR_NO_KEY  # no client key: as fr_gen_server_key
    std = keys.ctx(keys.key_blob)
    std.gen_server_key(SEED)
    sk, sb = std.export_server_key()
    loaded = keys.ctx()
    loaded.load_server_key(keys.ksk, keys.bsk)
    for c, (wk, wb) in ((std, (sk, sb)), (loaded, (keys.ksk, keys.bsk))):
        with pytest.raises(F.FheRegexError) as e:
            c.export_server_key_compact()
        assert e.value.code == F.ERR_INVALID and "compact" in str(e.value)
        k3, b3 = c.export_server_key()
        assert np.array_equal(k3, wk) and np.array_equal(b3, wb)
    # a compact context that takes a standard key forgets its mask key
    server.load_server_key(sk, sb)
    with pytest.raises(F.FheRegexError):
        server.export_server_key_compact()


def test_header_mutation_fuzz(keys):
    """200 seeded mutations of header bytes and of the length: refused, or a key whose
    compact re-export is the mutated blob (a changed mask key is another valid key)"""
    rng = np.random.default_rng(20251019 + keys.N)
    server = keys.ctx()
    server.load_server_key_compact(keys.blob)
    installed = keys.blob
    loaded = 0
    for it in range(200):
        kind = rng.integers(0, 3)
        blob = keys.blob
        if kind != 0:  # 1..3 header bytes
            head = bytearray(blob[:72])
            for pos in rng.integers(0, 72, rng.integers(1, 4)):
                head[pos] = int(rng.integers(0, 256))
            blob = bytes(head) + blob[72:]
        if kind != 1:  # the length
            cut = int(rng.choice([1, 7, 8, 64, 72, int(rng.integers(1, len(blob)))]))
            blob = blob[:len(blob) - cut] if rng.integers(0, 2) else blob + bytes(rng.integers(0, 256, min(cut, 4096),
                                                                                                 dtype=np.uint8))
        try:
            server.load_server_key_compact(blob)
        except F.FheRegexError as e:
            assert e.code == F.ERR_INVALID
            # (re-export of the 36 MB key after every refusal is test_refusals' job)
            continue
        loaded += 1
        installed = blob
        assert blob[:40] == keys.blob[:40] and len(blob) == len(keys.blob)
        assert server.export_server_key_compact() == blob
    assert server.export_server_key_compact() == installed
    assert loaded < 200
