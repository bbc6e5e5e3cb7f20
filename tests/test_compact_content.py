"""Compact (seeded) content ciphertexts on host-only contexts: both FFT points and the RNS ring.

A compact blob is "FRCCTXT1", k, N, first_block, n_blocks, a public mask key M = words 0..7
of chacha_block(K, stream 8, 0) and one u64 body per block (include/fheregex.h).  The masks
of block q are M's words at the standard encryptor's indices (first_block + q) kN + t of
stream 5; the noise is the standard encryptor's under the secret K.

Pins:
- sizes and header; the size query; the size function;
- the masks are M's stream, pinned through the oracle-pinned encryptor run under M;
- the noise is K's stream: phase - m 2^59 equals, as an exact integer, the residual of the
  standard encryption under K, block for block;
- M is the mask key of a compact server key generated under the same K;
- every char decrypts; fresh under the OS CSPRNG, reproducible under a key or a seed;
- a server context without a client key expands; the error codes of the neighbouring calls;
- every malformed blob is refused with ERR_INVALID; a mutated header is refused or expands
  to other words.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import fheregex as F

K = bytes((41 * i + 7) & 0xFF for i in range(32))  # a fixed 256-bit generator key
SEED = 0xC0DE5EED
POINTS = [(1, 2048, F.RING_FFT), (2, 1024, F.RING_FFT), (1, 2048, F.RING_RNS)]
FIRST = [0, 7, 2 ** 33 + 5]  # the last puts the ChaCha block counter above 32 bits
U = np.uint64


class Setup:
    def __init__(self, point, key_blob):
        k, N, ring = point
        self.k, self.N, self.ring = point
        self.p = F.default_params(k=k, N=N, ring=ring)
        self.client = F.Context(device=-1, params=self.p)
        self.client.load_client_key(key_blob)
        self.server = F.Context(device=-1, params=self.p)  # never sees a client key
        self.key_blob = key_blob
        self.L = k * N + 1


@pytest.fixture(scope="module", params=POINTS, ids=["k1n2048", "k2n1024", "rns"])
def su(request, key_blob):
    return Setup(request.param, key_blob)


def header(blob):
    magic, k, N, first, n = struct.unpack_from("<8siiQQ", blob, 0)
    return magic, k, N, first, n


def residual(s_big, lwes, msgs):
    """phase - m 2^59 of every block, mod 2^64 (numpy u64 arithmetic wraps)"""
    lw = lwes.reshape(-1, lwes.shape[-1])
    dot = lw[:, :-1][:, np.asarray(s_big, dtype=U) == 1].sum(axis=1, dtype=U)
    return lw[:, -1] - dot - (np.asarray(msgs, dtype=U) << U(59))


def str_msgs(s):
    return [(ord(c) >> (2 * b)) & 3 for c in s for b in range(4)]


def test_sizes_and_header(su):
    c = su.client
    for s in ("a", "0123456789abcdef"):
        blob = c.encrypt_str_compact(s, K)
        assert len(blob) == 64 + 32 * len(s) == c.compact_content_size(4 * len(s))
        assert header(blob) == (b"FRCCTXT1", su.k, su.N, 0, 4 * len(s))
        assert F.compact_content_mask_key(blob) == blob[32:64] and blob[:8] == F.COMPACT_CONTENT_MAGIC
        # size query, exact write into a larger buffer, refusal of a smaller one
        n = C.c_size_t()
        F._check(F.lib().fr_encrypt_str_compact_keyed(c.h, s.encode(), len(s), K, None, 0, C.byref(n)))
        assert n.value == len(blob)
        buf = C.create_string_buffer(b"\xA5" * (len(blob) + 16), len(blob) + 16)
        F._check(F.lib().fr_encrypt_str_compact_keyed(c.h, s.encode(), len(s), K, buf, len(blob) + 16, C.byref(n)))
        assert n.value == len(blob) and buf.raw[:len(blob)] == blob and buf.raw[len(blob):] == b"\xA5" * 16
        assert F.lib().fr_encrypt_str_compact_keyed(c.h, s.encode(), len(s), K, buf, len(blob) - 1,
                                                    C.byref(n)) == F.ERR_INVALID
    for nb in (1, 3, 5):
        for f in FIRST:
            blob = c.encrypt_blocks_compact(list(range(nb)), K, f)
            assert len(blob) == 64 + 8 * nb == c.compact_content_size(nb)
            assert header(blob) == (b"FRCCTXT1", su.k, su.N, f, nb)
    # the bodies are the expanded blocks' body words, in order
    blob = c.encrypt_blocks_compact([1, 2, 3], K, 7)
    assert np.array_equal(np.frombuffer(blob, dtype="<u8", offset=64), c.expand_compact_content(blob)[:, -1])
    with pytest.raises(ValueError):
        F.compact_content_mask_key(b"FRCCTXT0" + blob[8:])
    assert c.encrypt_str_compact("", K)[24:32] == bytes(8) and len(c.encrypt_str_compact("", K)) == 64
    with pytest.raises(F.FheRegexError) as e:
        c.compact_content_size(2 ** 40 + 1)
    assert e.value.code == F.ERR_INVALID


@pytest.mark.parametrize("first", FIRST)
@pytest.mark.parametrize("nb", [1, 3, 5])
def test_masks_and_noise(su, fixture_key, nb, first):
    c = su.client
    msgs = [(5 * q + nb + first) % 16 for q in range(nb)]
    blob = c.encrypt_blocks_compact(msgs, K, first)
    M = F.compact_content_mask_key(blob)
    assert M != K
    got = su.server.expand_compact_content(blob)  # no client key
    assert got.shape == (nb, su.L)
    # masks: the oracle-pinned encryptor under the public mask key, word for word
    under_m = c.encrypt_blocks(msgs, M, first)
    assert np.array_equal(got[:, :-1], under_m[:, :-1])
    # noise: the standard encryption under K has the same residual, as an exact integer
    std = c.encrypt_blocks(msgs, K, first)
    r_c, r_s = residual(fixture_key["s_big"], got, msgs), residual(fixture_key["s_big"], std, msgs)
    assert np.array_equal(r_c, r_s)
    assert not np.array_equal(got[:, :-1], std[:, :-1])  # and not K's masks
    # 8 sigma (P < 1.3e-15 a sample) and not all zero
    assert np.abs(r_c.view(np.int64)).max() <= 8 * su.p.glwe_sigma * 2.0 ** 64
    for q in range(nb):
        assert c.decode_block(got[q]) == msgs[q]


def test_every_message_value(su, fixture_key):
    c = su.client
    msgs = list(range(16))
    got = c.expand_compact_content(c.encrypt_blocks_compact(msgs, K, 3))
    assert [c.decode_block(x) for x in got] == msgs
    std = c.encrypt_blocks(msgs, K, 3)
    r = residual(fixture_key["s_big"], got, msgs)
    assert np.array_equal(r, residual(fixture_key["s_big"], std, msgs))
    assert np.abs(r.view(np.int64)).max() > 0


def test_mask_key_is_the_compact_server_keys(key_blob):
    """one derive_mask_key: M of a blob is the mask key of a compact server key under the same
    K (the compact server key is FFT-ring only; M does not depend on the params)"""
    c = F.Context(device=-1, params=F.default_params(k=2, N=1024))
    c.load_client_key(key_blob)
    c.gen_server_key(K, compact=True)
    M = F.compact_mask_key(c.export_server_key_compact())
    for k, N, ring in POINTS:
        e = F.Context(device=-1, params=F.default_params(k=k, N=N, ring=ring))
        e.load_client_key(key_blob)
        assert F.compact_content_mask_key(e.encrypt_str_compact("x", K)) == M


@pytest.mark.parametrize("s", ["Z", "fhe regex: [a-c]"])
def test_strings_decrypt(su, s):
    c = su.client
    assert len(s) in (1, 16)
    blob = c.encrypt_str_compact(s, K)
    w = su.server.expand_compact_content(blob).reshape(len(s), 4, su.L)
    assert "".join(chr(c.decrypt_radix(x)) for x in w) == s
    # the string form is the block form of its radix digits at first_block 0
    assert blob == c.encrypt_blocks_compact(str_msgs(s), K, 0)
    assert F.ClientKey(c).encrypt_str_compact(s, K) == blob
    # masks: encrypt_str under M
    assert np.array_equal(w[:, :, :-1], c.encrypt_str(s, F.compact_content_mask_key(blob))[:, :, :-1])


def test_fresh_and_reproducible(su):
    c = su.client
    s = "0123456789abcdef"
    a, b = c.encrypt_str_compact(s), c.encrypt_str_compact(s)  # OS CSPRNG
    assert F.compact_content_mask_key(a) != F.compact_content_mask_key(b)
    ba, bb = (np.frombuffer(x, dtype="<u8", offset=64) for x in (a, b))
    assert (ba != bb).all()
    assert a[:32] == b[:32]
    for blob in (a, b):
        w = c.expand_compact_content(blob).reshape(len(s), 4, su.L)
        assert "".join(chr(c.decrypt_radix(x)) for x in w) == s
    assert c.encrypt_str_compact(s, K) == c.encrypt_str_compact(s, K)
    assert c.encrypt_str_compact(s, SEED) == c.encrypt_str_compact(s, F.seed_key(SEED))
    assert c.encrypt_blocks_compact([1, 2], SEED, 9) == c.encrypt_blocks_compact([1, 2], F.seed_key(SEED), 9)
    assert c.encrypt_str_compact(s, SEED) != c.encrypt_str_compact(s, K)


def test_server_without_a_client_key(su):
    srv = su.server
    blob = su.client.encrypt_str_compact("abc", K)
    assert np.array_equal(srv.expand_compact_content(blob), su.client.expand_compact_content(blob))
    with pytest.raises(F.FheRegexError) as e:
        srv.encrypt_str_compact("abc", K)
    assert e.value.code == F.ERR_NO_KEY
    with pytest.raises(F.FheRegexError) as e:
        srv.encrypt_blocks_compact([1], K)
    assert e.value.code == F.ERR_NO_KEY
    with pytest.raises(ValueError):
        su.client.encrypt_str_compact("caf\xe9", K)
    with pytest.raises(ValueError):
        F.ClientKey(su.client).encrypt_str_compact("caf\xe9", K)
    n = C.c_size_t()
    assert F.lib().fr_encrypt_str_compact_keyed(su.client.h, b"caf\xe9", 4, K, None, 0,
                                                C.byref(n)) == F.ERR_NON_ASCII
    with pytest.raises(F.FheRegexError) as e:
        su.client.encrypt_blocks_compact([16], K)
    assert e.value.code == F.ERR_INVALID
    for up in (srv.upload_compact_str, srv.upload_compact_blocks, F.ServerKey(srv).upload_str):
        with pytest.raises(F.NoDevice):
            up(blob)


def expand_rc(ctx, blob, out_words=None):
    """fr_expand_compact_content's return code and words (None when refused)"""
    n = C.c_size_t()
    nb = max(0, len(blob) - 64) // 8 + 1
    out = np.zeros(nb * ctx.lwe_len if out_words is None else max(out_words, 1), dtype=np.uint64)
    rc = F.lib().fr_expand_compact_content(ctx.h, bytes(blob), len(blob), F._p(out),
                                           out.size if out_words is None else out_words, C.byref(n))
    return rc, (out[:n.value * ctx.lwe_len] if rc == F.FR_OK else None)


def upload_rc(ctx, blob, radix, cap=64):
    n = C.c_size_t()
    out = (C.c_uint32 * 64)()
    f = F.lib().fr_upload_compact_str if radix else F.lib().fr_upload_compact_blocks
    return f(ctx.h, bytes(blob), len(blob), out, cap, C.byref(n))


def test_refusals(su):
    c, srv = su.client, su.server
    blob = c.encrypt_blocks_compact([1, 2, 3, 0, 1, 2, 3, 0], K, 7)
    assert expand_rc(srv, blob)[0] == F.FR_OK

    def put(off, fmt, v):
        return blob[:off] + struct.pack(fmt, v) + blob[off + struct.calcsize(fmt):]

    ok, oN = (2, 1024) if (su.k, su.N) == (1, 2048) else (1, 2048)
    bad = [
        b"FRCCTXT2" + blob[8:], b"frcctxt1" + blob[8:], b"FRCSKEY1" + blob[8:],
        blob[:-1], blob + b"\0", blob[:-8], blob + bytes(8), blob[:63], b"", blob[:64 + 4],
        put(8, "<i", ok), put(12, "<i", oN), put(8, "<i", 0), put(12, "<i", -su.N),
        put(24, "<Q", 7), put(24, "<Q", 9), put(24, "<Q", 0), put(24, "<Q", 2 ** 61 + 8),
        put(16, "<Q", 2 ** 63), put(16, "<Q", 2 ** 40 - 7), put(16, "<Q", 2 ** 64 - 4),
    ]
    for b in bad:
        assert expand_rc(srv, b)[0] == F.ERR_INVALID, b[:32]
        # the uploads check the blob before they ask for the device
        assert upload_rc(srv, b, True) == F.ERR_INVALID
        assert upload_rc(srv, b, False) == F.ERR_INVALID
        with pytest.raises(F.FheRegexError) as e:
            srv.expand_compact_content(b)
        assert e.value.code == F.ERR_INVALID
    # the bound itself is allowed
    assert expand_rc(srv, put(16, "<Q", 2 ** 40 - 8))[0] == F.FR_OK
    # n_blocks % 4 != 0: a block blob, but no string
    odd = c.encrypt_blocks_compact([1, 2, 3, 0, 1], K, 0)
    assert expand_rc(srv, odd)[0] == F.FR_OK
    assert upload_rc(srv, odd, True) == F.ERR_INVALID
    assert upload_rc(srv, odd, False) == F.ERR_NO_DEVICE  # a good block blob: only the device is missing
    assert upload_rc(srv, blob, True) == F.ERR_NO_DEVICE
    # cap one short (8 blocks: 2 chars or 8 booleans), checked before the device is asked for
    assert upload_rc(srv, blob, True, cap=1) == F.ERR_INVALID
    assert upload_rc(srv, blob, False, cap=7) == F.ERR_INVALID
    assert upload_rc(srv, blob, True, cap=2) == F.ERR_NO_DEVICE
    assert upload_rc(srv, blob, False, cap=8) == F.ERR_NO_DEVICE
    # out_words one short
    L = srv.lwe_len
    assert expand_rc(srv, blob, out_words=8 * L - 1)[0] == F.ERR_INVALID
    rc, w = expand_rc(srv, blob, out_words=8 * L)
    assert rc == F.FR_OK and np.array_equal(w.reshape(8, L), srv.expand_compact_content(blob))
    # the other point's own blob
    other = F.Context(device=-1, params=F.default_params(k=ok, N=oN))
    other.load_client_key(su.key_blob)
    assert expand_rc(srv, other.encrypt_blocks_compact([1, 2, 3, 0], K, 0))[0] == F.ERR_INVALID
    # encryption past the index bound
    with pytest.raises(F.FheRegexError) as e:
        c.encrypt_blocks_compact([1, 2], K, 2 ** 40 - 1)
    assert e.value.code == F.ERR_INVALID
    assert len(c.encrypt_blocks_compact([1, 2], K, 2 ** 40 - 2)) == 80


def test_header_mutation_fuzz(su):
    """300 seeded single-byte header mutations: refused, or expanded to other words; none is
    silently taken for the original"""
    srv = su.server
    blob = su.client.encrypt_blocks_compact([3, 1, 2, 0], K, 5)
    orig = srv.expand_compact_content(blob).reshape(-1)
    rng = np.random.default_rng(20261019 + su.N + su.ring)
    accepted = 0
    for _ in range(300):
        pos = int(rng.integers(0, 64))
        v = int(rng.integers(0, 256))
        if v == blob[pos]:
            v ^= 0x80
        m = blob[:pos] + bytes([v]) + blob[pos + 1:]
        rc, w = expand_rc(srv, m)
        if rc != F.FR_OK:
            assert rc == F.ERR_INVALID and 0 <= pos < 32, pos
            continue
        accepted += 1
        # only first_block (16..23, within the bound) and the mask key can change and pass
        assert 16 <= pos < 24 or 32 <= pos < 64, pos
        assert w.shape == orig.shape and not np.array_equal(w, orig)
        assert np.array_equal(w.reshape(4, -1)[:, -1], orig.reshape(4, -1)[:, -1])
    assert accepted > 100  # half the header is mask key
