"""256-bit keyed and OS-seeded randomness for keys and encryption.

Every random draw of the library is ChaCha20 under one generator key (csrc/chacha.h):
32 bytes = the 8 little-endian key words (state words 4..11), the stream id in words
14..15 and a 64-bit block counter in words 12..13.  A 64-bit seed stands for the key
(seed lo, seed hi, six fixed words); `None` draws the key from the OS CSPRNG per call.

The CPU tests pin the keyed path three ways: to RFC 8439 through a ChaCha20 block function
written here, to the seeded path (which the oracle pins) through the seed's own key, and to
every one of the 8 key words through one-bit flips.  The GPU tests pin the kernels, which
take the key by value, to the host generator word for word."""
import ctypes as C
import struct
import time

import numpy as np
import pytest

import fheregex as F
import oracle_ffi as of

LEGACY_WORDS = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
# a key none of whose 8 words is a word of a seed's key
KEY = bytes(range(0xA0, 0xC0))
STREAM_ENC_MASK = 5
KEYED_SYMBOLS = ("fr_gen_client_key_keyed", "fr_gen_server_key_keyed", "fr_encrypt_blocks_keyed",
                 "fr_encrypt_str_keyed", "fr_encrypt_upload_str_keyed")
PARAM_POINTS = [(1, 2048), (2, 1024)]
PARAM_IDS = ["k1n2048", "k2n1024"]


def legacy_key(seed: int) -> bytes:
    """the 32 bytes a 64-bit seed has always stood for"""
    return struct.pack("<Q6I", seed, *LEGACY_WORDS)


def flipped(key: bytes, word: int, bit: int = 13) -> bytes:
    w = list(struct.unpack("<8I", key))
    w[word] ^= 1 << bit
    return struct.pack("<8I", *w)


# ---------------------------------------------------------------- ChaCha20, restated
def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha_blocks(key: bytes, stream: int, counters) -> np.ndarray:
    """ChaCha20 blocks [len(counters)][16] u32 (RFC 8439 rounds; state words 12..13 the
    64-bit counter, 14..15 the stream), vectorised over the counters."""
    ctr = np.asarray(counters, dtype=np.uint64)
    n = len(ctr)
    const = [np.full(n, v, dtype=np.uint32) for v in
             (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *struct.unpack("<8I", key))]
    tail = [(ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32),
            np.full(n, stream & 0xFFFFFFFF, dtype=np.uint32), np.full(n, stream >> 32, dtype=np.uint32)]
    init = const + tail
    x = [v.copy() for v in init]
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return np.stack([a + b for a, b in zip(x, init)], axis=1)


def stream_u64(key: bytes, stream: int, first: int, count: int) -> np.ndarray:
    """u64 numbers first .. first + count - 1 of a stream: number i is words
    (2 (i % 8), 2 (i % 8) + 1) of block i // 8"""
    b0, b1 = first // 8, (first + count - 1) // 8
    w = chacha_blocks(key, stream, np.arange(b0, b1 + 1, dtype=np.uint64)).astype(np.uint64)
    u = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(-1)
    return u[first - 8 * b0: first - 8 * b0 + count]


RFC8439_2_3_2 = [int(w, 16) for w in
                 ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()]


@pytest.fixture(scope="module")
def hctx(key_blob):
    """host-only context holding the golden client key"""
    ctx = F.Context(device=-1)
    ctx.load_client_key(key_blob)
    return ctx


@pytest.fixture(scope="module")
def s_big(key_blob):
    return of.parse_client_key(key_blob)["s_big"]


def fresh_ctx(key_blob, device=-1, k=1, N=2048, ring=None):
    ctx = F.Context(device=device, params=F.default_params(k=k, N=N, ring=ring))
    ctx.load_client_key(key_blob)
    return ctx


# ---------------------------------------------------------------- CPU
def test_external_anchor_rfc8439_and_mask_words(hctx):
    """the block function here is RFC 8439's, and the library's masks are its words"""
    # RFC 8439 2.3.2: key 00..1f, block counter 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00;
    # in this layout the counter is 0x0900000000000001 and the stream 0x4a000000
    got = chacha_blocks(bytes(range(32)), 0x4A000000, [0x0900000000000001])[0]
    assert [int(v) for v in got] == RFC8439_2_3_2
    assert not set(struct.unpack("<8I", KEY)) & set(LEGACY_WORDS)
    big = hctx.big
    for first_block in (0, 3):
        ct = hctx.encrypt_blocks([1, 2], KEY, first_block=first_block)
        for q in range(2):
            exp = stream_u64(KEY, STREAM_ENC_MASK, (first_block + q) * big, big)
            assert np.array_equal(ct[q, :big], exp), (first_block, q)


@pytest.mark.parametrize("seed", [0, 42, 2**64 - 1])
def test_legacy_key_equals_seed_client_side(hctx, seed):
    key = legacy_key(seed)
    assert F.seed_key(seed) == key
    blobs = []
    for s in (seed, key):
        ctx = F.Context(device=-1)
        ctx.gen_client_key(s)
        blobs.append(ctx.serialize_client_key())
    assert blobs[0] == blobs[1]
    assert np.array_equal(hctx.encrypt_str("Hi, regex!", key), hctx.encrypt_str("Hi, regex!", seed))
    msgs = [0, 3, 15, 7, 9]
    assert np.array_equal(hctx.encrypt_blocks(msgs, key, first_block=5), hctx.encrypt_blocks(msgs, seed, first_block=5))


@pytest.mark.parametrize("ring,seed", [(F.RING_FFT, 42), (F.RING_RNS, 2**64 - 1)], ids=["fft", "rns"])
def test_legacy_key_equals_seed_host_server_key(key_blob, ring, seed):
    keys = []
    for s in (seed, legacy_key(seed)):
        ctx = fresh_ctx(key_blob, ring=ring)
        ctx.gen_server_key(s)
        keys.append(ctx.export_server_key())
    assert np.array_equal(keys[0][0], keys[1][0])
    assert np.array_equal(keys[0][1], keys[1][1])


def test_all_256_key_bits_count(hctx):
    base_mask = int(hctx.encrypt_blocks([0], KEY)[0, 0])
    ctx = F.Context(device=-1)
    ctx.gen_client_key(KEY)
    base_ck = ctx.serialize_client_key()
    for word in range(8):
        key = flipped(KEY, word)
        assert int(hctx.encrypt_blocks([0], key)[0, 0]) != base_mask, word
        ctx.gen_client_key(key)
        assert ctx.serialize_client_key() != base_ck, word


def test_default_encryption_draws_from_the_os(hctx, s_big):
    big = hctx.big
    a, b = hctx.encrypt_str("abc"), hctx.encrypt_str("abc")
    assert a.shape == b.shape == (3, 4, big + 1)
    # 12 * kN positions; two independent uniform u64 coincide somewhere with p ~ 2^-50
    assert (a[..., :big] != b[..., :big]).all()
    assert (a[..., big] != b[..., big]).all()
    noise = []
    for ct in (a, b):
        assert bytes(hctx.decrypt_radix(ct[i]) for i in range(3)) == b"abc"
        e = []
        for i, ch in enumerate(b"abc"):
            for blk in range(4):
                m = (ch >> (2 * blk)) & 3
                phase = int(ct[i, blk, big]) - int(np.dot(ct[i, blk, :big], s_big).astype(np.uint64))
                v = (phase - (m << 59)) % 2**64
                e.append(v - 2**64 if v >= 2**63 else v)
        # glwe sigma 2^64 = 5.4e3: 2^30 is 2e5 sigma away, and 2^29 below the decoding bound
        assert max(abs(v) for v in e) < 2**30
        noise.append(e)
    # as a whole: two independent draws coincide in a single block about once in 20,000
    assert noise[0] != noise[1]


def test_default_client_keys_differ_and_load_back():
    blobs = []
    for _ in range(2):
        ctx = F.Context(device=-1)
        ctx.gen_client_key()
        blob = ctx.serialize_client_key()
        assert len(blob) == 38872
        back = F.Context(device=-1)
        back.load_client_key(blob)
        assert back.serialize_client_key() == blob
        ct = ctx.encrypt_str("k")
        assert back.decrypt_radix(ct[0]) == ord("k")
        blobs.append(blob)
    assert blobs[0] != blobs[1]


def test_gen_keys_and_client_encrypt_default_to_os_randomness():
    import inspect
    sig = inspect.signature(F.gen_keys).parameters
    assert sig["seed"].default is None and sig["client_seed"].default is None
    assert inspect.signature(F.ClientKey.encrypt_str).parameters["seed"].default is None
    ck1, sk1 = F.gen_keys(device=-1)
    ck2, sk2 = F.gen_keys(device=-1)
    assert ck1.serialize() != ck2.serialize()
    # one client key, two default server keys: fresh masks and bodies each time
    ck3, sk3 = F.gen_keys(ck1.serialize(), device=-1)
    k1, k3 = sk1.ctx.export_server_key()[0], sk3.ctx.export_server_key()[0]
    assert (k1 != k3).all()


def test_key_length_and_type_errors(hctx):
    for bad in (bytes(31), bytes(33), b""):
        for call in (lambda k: F.Context(device=-1).gen_client_key(k), hctx.gen_server_key,
                     lambda k: hctx.encrypt_str("a", k), lambda k: hctx.encrypt_blocks([1], k),
                     lambda k: hctx.encrypt_upload_str("a", k)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(TypeError):
        hctx.encrypt_str("a", 1.5)
    with pytest.raises(ValueError):
        hctx.encrypt_str("\xe9", KEY)  # FR_ERR_NON_ASCII


def test_keyed_preconditions(hctx):
    nokey = F.Context(device=-1)
    for key in (KEY, None):
        for call in (nokey.gen_server_key, lambda k: nokey.encrypt_str("a", k), lambda k: nokey.encrypt_blocks([1], k),
                     lambda k: nokey.encrypt_upload_str("a", k)):
            with pytest.raises(F.FheRegexError) as e:
                call(key)
            assert e.value.code == F.ERR_NO_KEY
        # device entries on a host-only context
        with pytest.raises(F.NoDevice):
            hctx.encrypt_upload_str("a", key)
        dev_only = F.Context(device=-1)
        dev_only.gen_client_key(7)
        dev_only.set_keygen(F.KEYGEN_DEVICE)
        with pytest.raises(F.NoDevice):
            dev_only.gen_server_key(key)
    # a null context
    L = F.lib()
    out = np.zeros(4 * hctx.lwe_len, dtype=np.uint64)
    h = (C.c_uint32 * 1)()
    m = (C.c_uint8 * 1)(1)
    assert L.fr_gen_client_key_keyed(None, KEY) == F.ERR_INVALID
    assert L.fr_gen_server_key_keyed(None, KEY) == F.ERR_INVALID
    assert L.fr_encrypt_blocks_keyed(None, m, 1, KEY, 0, F._p(out)) == F.ERR_INVALID
    assert L.fr_encrypt_str_keyed(None, b"a", 1, KEY, F._p(out)) == F.ERR_INVALID
    assert L.fr_encrypt_upload_str_keyed(None, b"a", 1, KEY, h) == F.ERR_INVALID


def test_keyed_symbols_everywhere():
    import os
    import re
    hdr = open(F.HEADER).read()
    doc = open(os.path.join(F.REPO, "INTEGRATION.md")).read()
    lib = C.CDLL(F.LIB_PATH)
    for sym in KEYED_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
        assert hasattr(lib, sym), sym
        assert sym in F._SIGS
        assert re.search(r"\bfn " + sym + r"\(", doc), sym


# ---------------------------------------------------------------- GPU
def _server_key(key_blob, device, where, seed, k, N):
    ctx = fresh_ctx(key_blob, device=device, k=k, N=N, ring=F.RING_FFT)
    ctx.set_keygen(where)
    t0 = time.perf_counter()
    ctx.gen_server_key(seed)
    dt = time.perf_counter() - t0
    return ctx.export_server_key(), dt


@pytest.mark.gpu
@pytest.mark.parametrize("kN", PARAM_POINTS, ids=PARAM_IDS)
def test_device_keygen_under_a_key_matches_host(key_blob, kN):
    """k_gen_ksk and k_gen_bsk<N> with all 8 key words other than a seed's"""
    k, N = kN
    (ksk, bsk), dt = _server_key(key_blob, 0, F.KEYGEN_DEVICE, KEY, k, N)
    (hk, hb), _ = _server_key(key_blob, -1, F.KEYGEN_HOST, KEY, k, N)
    print(f"device keygen (keyed, k={k} N={N}) {dt * 1e3:.1f} ms")
    assert np.array_equal(ksk, hk)
    assert np.array_equal(bsk, hb)


@pytest.mark.gpu
def test_device_keygen_legacy_key_equals_seed(key_blob):
    (k1, b1), _ = _server_key(key_blob, 0, F.KEYGEN_DEVICE, legacy_key(42), 1, 2048)
    (k2, b2), _ = _server_key(key_blob, 0, F.KEYGEN_DEVICE, 42, 1, 2048)
    assert np.array_equal(k1, k2)
    assert np.array_equal(b1, b2)


@pytest.mark.gpu
@pytest.mark.parametrize("kN", PARAM_POINTS, ids=PARAM_IDS)
def test_device_encryption_under_a_key_matches_host(key_blob, kN):
    k, N = kN
    ctx = fresh_ctx(key_blob, device=0, k=k, N=N, ring=F.RING_FFT)
    s = "a~ \x00Z"
    host = ctx.encrypt_str(s, KEY)
    dev = np.stack([ctx.download_radix(h) for h in ctx.encrypt_upload_str(s, KEY)])
    assert np.array_equal(dev, host)
    # every word of the kernel argument reaches the kernel
    seen = {host[0].tobytes()}
    for word in range(8):
        key = flipped(KEY, word)
        (h,) = ctx.encrypt_upload_str("a", key)
        got = ctx.download_radix(h)
        assert np.array_equal(got, ctx.encrypt_str("a", key)[0]), word
        seen.add(got.tobytes())
    assert len(seen) == 9


@pytest.mark.gpu
def test_default_keys_end_to_end(key_blob):
    ck, sk = F.gen_keys(device=0)
    for text, exp in (("xxabcx", 1), ("xxabxc", 0)):
        assert ck.decrypt(F.has_match(sk, ck.encrypt_str(text), "/abc/")) == exp, text
    ck2, sk2 = F.gen_keys(ck.serialize(), device=0)
    assert ck2.serialize() == ck.serialize()
    assert (sk.ctx.export_server_key()[0] != sk2.ctx.export_server_key()[0]).all()
    ctx = ck.ctx
    big = ctx.big
    a, b = (np.stack([ctx.download_radix(h) for h in ctx.encrypt_upload_str("xxabcx")]) for _ in range(2))
    assert (a[..., :big] != b[..., :big]).all()
    assert (a[..., big] != b[..., big]).all()
    for ct in (a, b):
        assert bytes(ctx.decrypt_radix(ct[i]) for i in range(6)) == b"xxabcx"
