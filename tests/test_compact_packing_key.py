"""The compact (seeded) packing key on host-only contexts, both FFT points.

A compact packing key is an ordinary packing key whose mask words are all ChaCha20 words of the
public mask key M = words 0..7 of chacha_block(K, stream 8, 0) at the standard generator's
indices, whose noise is the standard generator's under the secret K, and whose bodies are
rounded to 40 bits: b40 = ((B + 2^23) >> 24) mod 2^40, installed as b40 << 24 on the client as
on the server (include/fheregex.h).  On the wire: "FRCPKEY1", the eight
parameters, the gadget, the body bits, M, then a u32 plane (b40 >> 8) and a u8 plane (b40 & 0xFF).

Pins:
- the masks are M's stream 9 at (r k + j) N + t, M is K's stream 8;
- every body word has 24 zero low bits, and phase(compact row) - phase(standard row under K)
  lies in (-2^23, 2^23]: the two phases share K's noise and the message, so the difference is
  exactly the rounding -- the noise is K's and the rounding rule is the stated one;
- sizes, export -> load -> export, a keyless host context's full export, every refusal;
- a pack with the compact key decrypts and stays under the phase-error bound of
  test_packed_results.py (derived there: sqrt(sigma_in^2 + (2^47.5)^2), max < 2^52); the
  rounding adds std 2^39.2 at n = N, a 2^-16 share of the bound's variance;
- gen_keys(packing_compact=True) -> save_compact -> load_compact.
"""
import os
import struct

import numpy as np
import pytest

import fheregex as F
from test_keyed_rng import chacha_blocks, stream_u64
from test_packed_results import DELTA_LOG, negacyclic_phase, s_big, signed

K = bytes((29 * i + 5) & 0xFF for i in range(32))  # a fixed 256-bit generator key
POINTS = [(1, 2048), (2, 1024)]
SIZES = {(1, 2048): 62_914_656, (2, 1024): 31_457_376}
STREAM_MASK_KEY, STREAM_PKSK_MASK = 8, 9
U = np.uint64


def host(point, key_blob=None):
    k, N = point
    ctx = F.Context(device=-1, params=F.default_params(k=k, N=N))
    if key_blob is not None:
        if k == 1:
            ctx.load_client_key(key_blob)
        else:
            ctx.gen_client_key(7)
    return ctx


class Keys:
    """per point, shared read-only: a client holding the compact-generated key, and its blob"""

    def __init__(self, point, key_blob):
        self.point = point
        self.k, self.N = point
        self.KD = 3 * self.k * self.N
        self.client = host(point, key_blob)
        self.client.gen_packing_key(K, compact=True)
        self.blob = self.client.export_packing_key_compact()
        self.M = F.compact_packing_mask_key(self.blob)
        self.rows_at = sorted({0, 1, 2, self.KD // 2 + 1, self.KD - 1})


@pytest.fixture(scope="module", params=POINTS, ids=["k1n2048", "k2n1024"])
def keys(request, key_blob):
    return Keys(request.param, key_blob)


def planes(keys, blob):
    """(b40 of every body word) [3kN][N] from a blob's two planes"""
    n = keys.KD * keys.N
    hi = np.frombuffer(blob, dtype="<u4", count=n, offset=96).astype(U)
    lo = np.frombuffer(blob, dtype=np.uint8, count=n, offset=96 + 4 * n).astype(U)
    return ((hi << U(8)) | lo).reshape(keys.KD, keys.N)


# ------------------------------------------------------------------ masks
def test_masks_are_the_mask_keys_stream(keys):
    k, N = keys.point
    assert keys.M == chacha_blocks(K, STREAM_MASK_KEY, [0])[0][:8].astype("<u4").tobytes()
    assert keys.M == bytes(keys.blob[56:88]) and keys.M != K
    for r in keys.rows_at:
        row = keys.client.gen_packing_rows(K, r, r + 1, compact=True)[0]
        for j in range(k):
            assert np.array_equal(row[j * N:(j + 1) * N], stream_u64(keys.M, STREAM_PKSK_MASK, (r * k + j) * N, N)), (r, j)


# ------------------------------------------------------------------ bodies
def test_bodies_are_the_standard_bodies_rounded(keys):
    k, N = keys.point
    s = s_big(keys.client)
    b40 = planes(keys, keys.blob)
    for r in keys.rows_at:
        row = keys.client.gen_packing_rows(K, r, r + 1, compact=True)[0]
        std = keys.client.gen_packing_rows(K, r, r + 1)[0]  # masks and noise under K
        assert not (row[k * N:] & U(0xFFFFFF)).any(), r
        assert np.array_equal(row[k * N:] >> U(24), b40[r]), r  # the installed key is the blob's
        rho = signed(negacyclic_phase(row, s, k, N) - negacyclic_phase(std, s, k, N))
        assert rho.min() > -2 ** 23 and rho.max() <= 2 ** 23, (r, int(rho.min()), int(rho.max()))
        assert np.abs(rho).max() > 2 ** 20  # (N uniform draws: a rounding did take place)


# ------------------------------------------------------------------ the wire
def test_sizes_and_header(keys):
    p = keys.client.params
    want = 96 + 5 * keys.KD * keys.N
    assert want == SIZES[keys.point]
    assert len(keys.blob) == keys.client.packing_key_compact_size() == want
    assert bytes(keys.blob[:8]) == b"FRCPKEY1"
    assert struct.unpack("<12i", bytes(keys.blob[8:56])) == (p.k, p.N, p.n, p.ks_base_log, p.ks_level, p.pbs_base_log,
                                                            p.pbs_level, F.RING_FFT, 7, 3, 40, 0)
    assert bytes(keys.blob[88:96]) == bytes(8)
    assert host(keys.point).packing_key_compact_size() == want  # needs no key


def trivial_pack(ctx):
    one = ctx.not_(ctx.or_many([]))
    return ctx.pack_bools_words([one, ctx.or_many([]), one])


def test_round_trip_and_keyless_host(keys):
    k, N = keys.point
    server = host(keys.point)  # no client key
    with pytest.raises(F.FheRegexError):
        server.export_packing_key_compact()  # no packing key at all
    server.load_packing_key_compact(keys.blob)
    assert np.array_equal(server.export_packing_key_compact(), keys.blob)
    # what it installed is the generating context's key, word for word
    full = server.export_packing_key()
    assert np.array_equal(full, keys.client.export_packing_key())
    rows = np.frombuffer(full, dtype="<u8", offset=48).reshape(keys.KD, (k + 1) * N)
    for r in keys.rows_at:
        assert np.array_equal(rows[r], keys.client.gen_packing_rows(K, r, r + 1, compact=True)[0]), r
    # ... and an ordinary packing key: the full blob loads through the existing entry, after
    # which the compact export is refused (that install's masks could be anything)
    plain = host(keys.point)
    plain.load_packing_key_compact(keys.blob.tobytes())  # bytes as well as arrays
    plain.load_packing_key(full)
    assert np.array_equal(plain.export_packing_key(), full)
    with pytest.raises(F.FheRegexError) as e:
        plain.export_packing_key_compact()
    assert e.value.code == F.ERR_INVALID and "not generated in compact form" in str(e.value)
    plain.load_packing_key_compact(keys.blob)  # and back
    assert np.array_equal(plain.export_packing_key_compact(), keys.blob)


def test_compact_export_of_a_standard_key_is_refused(keys, key_blob):
    c = host(keys.point, key_blob)
    c.load_packing_key(keys.client.export_packing_key())
    with pytest.raises(F.FheRegexError) as e:
        c.export_packing_key_compact()
    assert e.value.code == F.ERR_INVALID and "not generated in compact form" in str(e.value)
    # a standard generation over a compact key clears the mark too (rows by range: the mark
    # is the context's, so the small default-point generation is enough)
    if keys.point == POINTS[0]:
        c.gen_packing_key(K, compact=True)
        assert len(c.export_packing_key_compact()) == SIZES[keys.point]
        c.gen_packing_key(K)
        with pytest.raises(F.FheRegexError):
            c.export_packing_key_compact()


def test_refusals_leave_the_installed_key(keys):
    server = host(keys.point)
    server.load_packing_key_compact(keys.blob)
    before = trivial_pack(server)
    blob = keys.blob.copy()

    def refused(bad, what):
        with pytest.raises(F.FheRegexError) as e:
            server.load_packing_key_compact(bad)
        assert e.value.code == F.ERR_INVALID, what
        assert np.array_equal(trivial_pack(server), before), what

    # the magic, each of the eight parameters, the gadget's base and levels, the body bits,
    # the reserved word, every pad byte
    fields = [(0, "magic"), (7, "magic")] + [(8 + 4 * i, f"param {i}") for i in range(8)]
    fields += [(40, "base"), (44, "levels"), (48, "body bits"), (52, "reserved"), (55, "reserved")]
    fields += [(at, "pad") for at in range(88, 96)]
    for at, what in fields:
        keep = blob[at]
        blob[at] = keep ^ 1
        refused(blob, (what, at))
        blob[at] = keep
    for bits in (32, 48, 64):
        blob[48] = bits
        refused(blob, bits)
    blob[48] = 40
    assert np.array_equal(blob, keys.blob)
    refused(blob[:-1], "one byte short")
    refused(np.append(blob, np.uint8(0)), "one byte long")
    refused(blob[:96], "header alone")
    refused(blob[:95], "short header")
    # the other point's blob, at its own length
    other = host(POINTS[1] if keys.point == POINTS[0] else POINTS[0])
    with pytest.raises(F.FheRegexError) as e:
        other.load_packing_key_compact(keys.blob)
    assert e.value.code == F.ERR_INVALID
    # a full blob through the compact entry and the reverse
    with pytest.raises(F.FheRegexError):
        server.load_packing_key(keys.blob)
    # the key is still the one it was
    assert np.array_equal(server.export_packing_key_compact(), keys.blob)


def test_reproducible_and_fresh(keys, key_blob):
    """rows by range: the same key gives the same words, an int seed stands for its 32 bytes,
    and two OS-keyed generations share neither masks nor mask key"""
    c = keys.client
    assert np.array_equal(c.gen_packing_rows(K, 1, 3, compact=True)[1], c.gen_packing_rows(K, 2, 3, compact=True)[0])
    assert np.array_equal(c.gen_packing_rows(5, 0, 1, compact=True), c.gen_packing_rows(F.seed_key(5), 0, 1, compact=True))
    a, b = c.gen_packing_rows(None, 0, 1, compact=True), c.gen_packing_rows(None, 0, 1, compact=True)
    assert not (a[:, :keys.k * keys.N] == b[:, :keys.k * keys.N]).any()
    with pytest.raises(F.FheRegexError) as e:
        host(keys.point).gen_packing_rows(K, 0, 1, compact=True)  # no client key
    assert e.value.code == F.ERR_NO_KEY
    with pytest.raises(F.FheRegexError) as e:
        host(keys.point).gen_packing_key(K, compact=True)
    assert e.value.code == F.ERR_NO_KEY


# ------------------------------------------------------------------ use and noise
def test_pack_decrypts_under_the_derived_bound(key_blob):
    """default point, fixture key: n = 33 fresh encryptions packed with the compact-generated
    key; the numbers of test_packed_results.py's test_decrypt_and_phase_error"""
    c = host(POINTS[0], key_blob)
    c.gen_packing_key(K, compact=True)
    n = 33
    rng = np.random.default_rng(100 + n)
    bits = rng.integers(0, 2, n).astype(np.uint8)
    lwes = c.encrypt_blocks(bits, seed=77).reshape(n, -1)
    words = c.pack_lwes(lwes)
    blob = b"FRPKRES1" + struct.pack("<iiQ", 1, 2048, n) + words.tobytes()
    assert c.decrypt_packed(blob) == list(bits)
    s = s_big(c)
    want = bits.astype(np.int64) << DELTA_LOG
    e_in = signed(lwes[:, -1] - (lwes[:, :-1] * s.astype(U)).sum(axis=1, dtype=U)) - want
    ph = signed(negacyclic_phase(words, s, 1, 2048))
    e_out = ph[:n] - want
    sigma_in = float(np.sqrt(np.mean(e_in.astype(np.float64) ** 2)))
    sigma_out = float(np.sqrt(np.mean(e_out.astype(np.float64) ** 2)))
    bound = np.sqrt(sigma_in ** 2 + (2.0 ** 47.5) ** 2)
    print(f"n={n}: sigma_in 2^{np.log2(sigma_in):.2f}, sigma_out 2^{np.log2(sigma_out):.2f}, bound 2^{np.log2(bound):.2f}")
    assert sigma_out < bound
    assert np.abs(e_out).max() < 2 ** 52
    assert np.abs(ph[n:]).max() < 2 ** 52


# ------------------------------------------------------------------ the Python surface
def test_gen_keys_and_key_files(key_blob, tmp_path):
    ck, sk = F.gen_keys(key_blob, seed=3, device=-1, compact=True, packing=True, packing_seed=K, packing_compact=True)
    a, b = str(tmp_path / "sk.blob"), str(tmp_path / "pk.blob")
    sk.save_compact(a, b)
    assert os.path.getsize(b) == SIZES[POINTS[0]]
    back = F.ServerKey.load_compact(a, device=-1, packing_path=b)
    assert np.array_equal(back.ctx.export_packing_key_compact(), sk.ctx.export_packing_key_compact())
    assert back.ctx.export_server_key_compact() == sk.ctx.export_server_key_compact()
    one, zero = back.ctx.not_(back.ctx.or_many([])), back.ctx.or_many([])
    assert ck.ctx.decrypt_packed(back.pack_bools([one, zero, one, one])) == [1, 0, 1, 1]
    plain = F.ServerKey.load_compact(a, device=-1)  # the first file alone is what it was
    with pytest.raises(F.FheRegexError):
        plain.ctx.export_packing_key()
    sk.save_compact(a)
    # today's compact=True, packing=True keeps giving a standard packing key
    _, std = F.gen_keys(key_blob, seed=3, device=-1, compact=True, packing=True, packing_seed=K)
    assert np.array_equal(np.frombuffer(std.ctx.export_packing_key(), dtype="<u8", offset=48)[:4096],
                          std.ctx.gen_packing_rows(K, 0, 1)[0])
    with pytest.raises(F.FheRegexError):
        std.ctx.export_packing_key_compact()
