"""Private search, host side (include/fheregex.h): the needle blob "FRNEEDL1", its selectors
(GLWE encryptions of the direct test polynomial of a 16-entry 0/1 table), needle_masks, the
lowering of fr_find / fr_find_starts (fr_schedule_find) and its plaintext evaluation
(fr_plain_find).  No device: the GPU side is tests/test_private_needle_gpu.py.

The mask words are pinned to a ChaCha20 written out here (RFC 8439 rounds, the 64-bit block
counter and the stream id in the nonce words, chacha.h): stream 11 under the public mask key
M = words 0..7 of block 0 of stream 8 under the generator key K."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import fheregex as F
import needle_limits as nl

K = bytes((41 * i + 7) & 0xFF for i in range(32))  # a fixed 256-bit generator key
HEADER = 64
U = np.uint64
STREAM_MASK_KEY, STREAM_NEEDLE_MASK = 8, 11
TABLES = [1 << 3, (1 << 4) | (1 << 6), 0xFFFF, 0, 1, 1 << 15]  # one bit, two bits, all, none, bit 0, bit 15


def chacha_block(key32: bytes, stream: int, counter: int):
    def rotl(a, b):
        return ((a << b) | (a >> (32 - b))) & 0xFFFFFFFF

    def qr(x, a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 7)

    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + list(struct.unpack("<8I", key32)) + [
        counter & 0xFFFFFFFF, counter >> 32, stream & 0xFFFFFFFF, stream >> 32]
    x = list(init)
    for _ in range(10):
        qr(x, 0, 4, 8, 12), qr(x, 1, 5, 9, 13), qr(x, 2, 6, 10, 14), qr(x, 3, 7, 11, 15)
        qr(x, 0, 5, 10, 15), qr(x, 1, 6, 11, 12), qr(x, 2, 7, 8, 13), qr(x, 3, 4, 9, 14)
    return [(a + b) & 0xFFFFFFFF for a, b in zip(x, init)]


def stream_u64(key32: bytes, stream: int, idx: int) -> int:
    w = chacha_block(key32, stream, idx // 8)
    return w[2 * (idx % 8)] | (w[2 * (idx % 8) + 1] << 32)


def direct_poly(N, table):
    """V(lut) of test_poly<N>(t, direct = true, lut): boxes of N/16 recentred by half a box,
    -lut[0] in the last half box, lut[s] 2^59"""
    mm = (np.arange(N) + N // 32) // (N // 16)
    bit = lambda s: ((table >> s) & 1) << 59  # noqa: E731
    return np.array([bit(int(s)) if s < 16 else -bit(0) % 2 ** 64 for s in mm], dtype=U)


class Setup:
    def __init__(self, k, N, key_blob):
        self.k, self.N = k, N
        self.p = F.default_params(k=k, N=N, ring=F.RING_FFT)
        self.client = F.Context(device=-1, params=self.p)
        if k == 1:
            self.client.load_client_key(key_blob)  # the fixture key
        else:
            self.client.gen_client_key(7)
        self.server = F.Context(device=-1, params=self.p)  # never sees a client key


@pytest.fixture(scope="module", params=[(1, 2048), (2, 1024)], ids=["k1n2048", "k2n1024"])
def su(request, key_blob):
    return Setup(*request.param, key_blob)


def rc_expand(ctx, blob):
    m = C.c_size_t()
    return F.lib().fr_expand_needle(ctx.h, bytes(blob), len(blob), None, 0, C.byref(m))


# ------------------------------------------------------------------ blob
def test_size_formula_and_header(su):
    c = su.client
    for m in (1, 3, 64):
        assert c.needle_size(m) == HEADER + 16 * m * su.N
    assert c.needle_size(1) == HEADER + (32768 if su.k == 1 else 16384)
    blob = c.encrypt_needle(F.needle_masks("abc"), K)
    assert len(blob) == c.needle_size(3)
    magic, k, N, m = struct.unpack_from("<8siiQ", blob, 0)
    assert (magic, k, N, m) == (b"FRNEEDL1", su.k, su.N, 3) and blob[56:64] == bytes(8)
    assert blob[24:56] == struct.pack("<8I", *chacha_block(K, STREAM_MASK_KEY, 0)[:8])  # M = derive_mask_key(K)
    # the bodies are the expanded selectors' body polynomials, in order
    w = su.server.expand_needle(blob)
    assert w.shape == (6, su.k + 1, su.N)
    assert np.array_equal(np.frombuffer(blob, dtype="<u8", offset=HEADER).reshape(6, su.N), w[:, -1])
    # size query, a larger buffer, a smaller one
    arr = (C.c_uint16 * 6)(*[v for lh in F.needle_masks("abc") for v in lh])
    n = C.c_size_t()
    F._check(F.lib().fr_encrypt_needle_keyed(c.h, arr, 3, K, None, 0, C.byref(n)))
    assert n.value == len(blob)
    buf = C.create_string_buffer(b"\xA5" * (len(blob) + 16), len(blob) + 16)
    F._check(F.lib().fr_encrypt_needle_keyed(c.h, arr, 3, K, buf, len(blob) + 16, C.byref(n)))
    assert buf.raw[:len(blob)] == blob and buf.raw[len(blob):] == b"\xA5" * 16
    assert F.lib().fr_encrypt_needle_keyed(c.h, arr, 3, K, buf, len(blob) - 1, C.byref(n)) == F.ERR_INVALID


def test_refusals(su):
    c, s = su.client, su.server
    blob = c.encrypt_needle(F.needle_masks("ab"), K)
    assert rc_expand(s, blob) == F.FR_OK

    def put(off, fmt, v):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)

    bad = {
        "truncated": blob[:-8],
        "one byte short": blob[:-1],
        "over-long": blob + bytes(8),
        "header only": blob[:HEADER],
        "shorter than the header": blob[:40],
        "magic": b"FRNEEDL0" + blob[8:],
        "content's magic": b"FRCCTXT1" + blob[8:],
        "k": put(8, "<i", 3 - su.k),
        "N": put(12, "<i", su.N // 2),
        "m = 0": put(16, "<Q", 0),
        "m = 65": put(16, "<Q", 65),
        "m = 3 in a blob of 2": put(16, "<Q", 3),
        "m = 2^61": put(16, "<Q", 2 ** 61),
        "pad": put(56, "<Q", 1),
    }
    for name, b in bad.items():
        assert rc_expand(s, b) == F.ERR_INVALID, name
    # a well-formed blob of 65 characters' length is refused by m alone
    long = put(16, "<Q", 65)[:HEADER] + bytes(16 * 65 * su.N)
    assert rc_expand(s, long) == F.ERR_INVALID
    n = C.c_size_t()
    for m in (0, 65):
        assert F.lib().fr_needle_size(c.h, m, C.byref(n)) == F.ERR_INVALID
        arr = (C.c_uint16 * 130)()
        assert F.lib().fr_encrypt_needle_keyed(c.h, arr, m, K, None, 0, C.byref(n)) == F.ERR_INVALID
    # too few words to expand into; a server needs no key, a client without one cannot encrypt
    words = np.zeros(4 * (su.k + 1) * su.N - 1, dtype=U)
    assert F.lib().fr_expand_needle(s.h, blob, len(blob), F._p(words), words.size, C.byref(n)) == F.ERR_INVALID
    arr = (C.c_uint16 * 2)(1, 1)
    assert F.lib().fr_encrypt_needle_keyed(s.h, arr, 1, K, None, 0, C.byref(n)) == F.ERR_NO_KEY
    # a host-only context has no device to upload to
    h = C.c_void_p()
    assert F.lib().fr_upload_needle(s.h, blob, len(blob), C.byref(h)) == F.ERR_NO_DEVICE


def test_rns_ring_refuses(key_blob):
    c = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_RNS))
    c.load_client_key(key_blob)
    arr = (C.c_uint16 * 2)(1, 1)
    n = C.c_size_t()
    assert F.lib().fr_encrypt_needle_keyed(c.h, arr, 1, K, None, 0, C.byref(n)) == F.ERR_INVALID
    assert "FFT ring only" in F.lib().fr_last_error().decode()
    fft = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_FFT))
    fft.load_client_key(key_blob)
    assert rc_expand(c, fft.encrypt_needle([(1, 1)], K)) == F.ERR_INVALID


# ------------------------------------------------------------------ selectors
def test_selector_phase_is_the_test_polynomial(su):
    """fr_expand_needle then fr_packed_phase: V(lut) coefficient by coefficient, within 2^16
    (12 sigma of sigma_glwe = 2^12.4 at k = 1; at most 2 * 3 * 2048 samples)"""
    c = su.client
    masks = [(TABLES[0], TABLES[1]), (TABLES[2], TABLES[3]), (TABLES[4], TABLES[5])]
    blob = c.encrypt_needle(masks, K)
    w = su.server.expand_needle(blob)
    flat = [t for lh in masks for t in lh]
    worst = 0
    for q, table in enumerate(flat):
        err = (c.packed_phase(w[q].reshape(-1)) - direct_poly(su.N, table)).view(np.int64)
        worst = max(worst, int(np.abs(err).max()))
        assert np.abs(err).max() < 2 ** 16, (q, hex(table), int(np.abs(err).max()))
        assert err.any()  # and there is noise
    print("largest selector phase error: 2^%.1f" % np.log2(worst))


def test_mask_words_are_the_mask_key_stream(su):
    """mask word t of mask polynomial c of selector q = u64 number (q k + c) N + t of stream 11
    under M; nothing of K's own stream"""
    blob = su.client.encrypt_needle([(1, 2), (4, 8)], K)
    M = blob[24:56]
    assert M != K
    w = su.server.expand_needle(blob)
    k, N = su.k, su.N
    for q, cc, t in [(0, 0, 0), (0, 0, 1), (0, 0, 7), (0, 0, 8), (0, k - 1, N - 1), (1, 0, 0), (2, k - 1, 5),
                     (3, 0, N - 1), (3, k - 1, N - 1), (1, k - 1, 1000)]:
        idx = (q * k + cc) * N + t
        assert int(w[q, cc, t]) == stream_u64(M, STREAM_NEEDLE_MASK, idx), (q, cc, t)
        assert int(w[q, cc, t]) != stream_u64(K, STREAM_NEEDLE_MASK, idx)
    # a whole polynomial, block by block
    want = []
    for b in range(N // 8):
        ws = chacha_block(M, STREAM_NEEDLE_MASK, (2 * k * N) // 8 + b)  # selector 2, polynomial 0
        want += [ws[2 * i] | (ws[2 * i + 1] << 32) for i in range(8)]
    assert [int(v) for v in w[2, 0]] == want


def test_keyed_is_reproducible_and_os_keys_are_fresh(su):
    c = su.client
    masks = F.needle_masks("ab")
    assert c.encrypt_needle(masks, K) == c.encrypt_needle(masks, K)
    assert c.encrypt_needle(masks, 5) == c.encrypt_needle(masks, 5) != c.encrypt_needle(masks, 6)
    a, b = c.encrypt_needle(masks), c.encrypt_needle(masks)  # NULL key: the OS CSPRNG
    assert a[24:56] != b[24:56]
    ba, bb = np.frombuffer(a, dtype="<u8", offset=HEADER), np.frombuffer(b, dtype="<u8", offset=HEADER)
    assert (ba != bb).all()
    for blob in (a, b):  # both still encrypt the needle
        w = su.server.expand_needle(blob)
        err = (c.packed_phase(w[0].reshape(-1)) - direct_poly(su.N, masks[0][0])).view(np.int64)
        assert np.abs(err).max() < 2 ** 16


# ------------------------------------------------------------------ needle_masks
def test_needle_masks():
    assert F.needle_masks("aB?", ignore_case=True, any_char="?") == [
        (1 << 1, 1 << 4 | 1 << 6), (1 << 2, 1 << 4 | 1 << 6), (0xFFFF, 0xFFFF)]
    assert F.needle_masks("aB?") == [(1 << 1, 1 << 6), (1 << 2, 1 << 4), (1 << 15, 1 << 3)]
    assert F.needle_masks("z[", ignore_case=True) == [(1 << 10, 1 << 5 | 1 << 7), (1 << 11, 1 << 5)]  # '[' is no letter
    assert F.needle_masks("@`", ignore_case=True) == [(1, 1 << 4), (1, 1 << 6)]
    assert F.needle_masks(b"\x00\xff") == [(1, 1), (1 << 15, 1 << 15)]


# ------------------------------------------------------------------ lowering
def content_ref(pos, blk):
    return -1 - (4 * pos + blk)


@pytest.mark.parametrize("n_chars,m", [(16, 1), (16, 3), (16, 8), (16, 9), (5, 5), (4, 5)])
@pytest.mark.parametrize("starts", [False, True])
def test_schedule(n_chars, m, starts):
    S = F.schedule_find(n_chars, m, starts=starts)
    fit = max(n_chars - m + 1, 0)
    if fit == 0:  # (4, 5): no job, the constant 0
        assert S.jobs == [] and S.level_off == [0]
        assert S.parts == ([(-1, 0, 0)] * n_chars if starts else [(-1, 0, 0)])
        return
    # level 1: exactly 2 m S selector jobs, start by start, character by character, low nibble first
    assert S.level_off[1] == 2 * m * fit
    lvl1 = S.jobs[:S.level_off[1]]
    at = 0
    for p in range(fit):
        for i in range(m):
            for h in range(2):
                j = lvl1[at]
                assert (j.kind, j.n_out, j.n_in, j.offset) == (F.JOB_ACC, 1, 2, 0)
                assert struct.unpack("<I", bytes(j.lut[0][:4]))[0] == 2 * i + h and not any(j.lut[0][4:])
                assert (j.in_ref[0], j.in_w[0]) == (content_ref(p + i, 2 * h + 1), 4)
                assert (j.in_ref[1], j.in_w[1]) == (content_ref(p + i, 2 * h), 1)
                at += 1
    assert len({j.out_gate[0] for j in lvl1}) == len(lvl1)  # one program gate each
    rest = S.jobs[S.level_off[1]:]
    assert all(j.kind == F.JOB_SIGN for j in rest)
    # the AND of a start: one gate for 2 m <= 16, else a balanced tree
    lvl2 = S.jobs[S.level_off[1]:S.level_off[2]]
    if 2 * m <= 16:
        assert len(lvl2) == fit and all(j.n_in == 2 * m and j.offset == 1 - 4 * m for j in lvl2)
        and_levels = 1
    else:
        assert m == 9 and len(lvl2) == 2 * fit and all(j.n_in == 9 and j.offset == 1 - 18 for j in lvl2)
        lvl3 = S.jobs[S.level_off[2]:S.level_off[3]]
        assert len(lvl3) == fit and all(j.n_in == 2 and j.offset == -3 for j in lvl3)
        and_levels = 2
    if starts:
        assert len(S.level_off) - 1 == 1 + and_levels
        assert len(S.parts) == n_chars
        tops = [g for g, w, c in S.parts[:fit]]
        assert all((w, c) == (1, 0) for g, w, c in S.parts[:fit]) and len(set(tops)) == fit
        assert S.parts[fit:] == [(-1, 0, 0)] * (n_chars - fit)  # a start that cannot fit: the constant
    else:
        or_jobs = S.jobs[S.level_off[1 + and_levels]:]
        if fit == 1:
            assert or_jobs == []
        else:
            assert len(or_jobs) == 1 and or_jobs[0].n_in == fit and or_jobs[0].offset == -1
        assert len(S.parts) == 1 and S.parts[0][1:] == (1, 0)


def test_schedule_bounds():
    nj = C.c_size_t()
    outs = (C.c_int32 * 3)()
    for m in (0, 65):
        assert F.lib().fr_schedule_find(16, m, 0, 16, 0, None, 0, C.byref(nj), None, 0, C.byref(nj), outs, 1,
                                        C.byref(nj)) == F.ERR_INVALID
    assert len(F.schedule_find(80, 64).jobs) > 0
    # find reads only the starts that fit: a range far past the content is the range cut there
    far = F.schedule_find(16, 3, 2, 16)
    nl, ns = C.c_size_t(), C.c_size_t()
    F._check(F.lib().fr_schedule_find(16, 3, 2, 2 ** 63, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1,
                                      C.byref(ns)))
    assert (nj.value, nl.value, ns.value) == (len(far.jobs), len(far.level_off) - 1, 1)
    # one output per start: at most 2^24 of them
    assert F.lib().fr_schedule_find(16, 3, 0, 2 ** 24 + 1, 1, None, 0, C.byref(nj), None, 0, C.byref(nl), outs,
                                    2 ** 24 + 1, C.byref(ns)) == F.ERR_INVALID
    any_ = C.c_int32()
    masks = (C.c_uint16 * 2)(1, 1)
    buf = (C.c_uint8 * 1)()
    assert F.lib().fr_plain_find(b"abc", 3, masks, 1, 0, 2 ** 63, buf, C.byref(any_)) == F.ERR_INVALID
    # a range: only its starts; the OR over more than 16 starts is a tree
    S = F.schedule_find(40, 2, 3, 30)
    assert S.level_off[1] == 4 * 27 and len(S.jobs[S.level_off[2]:S.level_off[3]]) == 2


def py_find(content: bytes, masks, lo, hi):
    m = len(masks)
    out = []
    for p in range(lo, hi):
        ok = p + m <= len(content) and all(
            (masks[i][0] >> (content[p + i] & 15)) & 1 and (masks[i][1] >> (content[p + i] >> 4)) & 1 for i in range(m))
        out.append(int(ok))
    return out


def test_plain_find_against_python():
    """200 seeded random (content over a 4-letter alphabet, needle, range) cases, lengths 1..24,
    with ignore_case and wildcards: every start and the OR; the literal cases also against
    bytes.find over every start"""
    rng = random.Random(20240611)
    hits = 0
    for case in range(200):
        n, m = rng.randint(1, 24), min(rng.randint(1, 24), rng.randint(1, 24))
        content = bytes(rng.choice(b"abAB") for _ in range(n))
        if rng.random() < 0.7 and m <= n:  # a needle cut from the content, so that matches occur
            at = rng.randint(0, n - m)
            needle = bytearray(content[at:at + m])
        else:
            needle = bytearray(rng.choice(b"abAB") for _ in range(m))
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
        starts, any_ = F.plain_find(content, masks, lo, hi)
        want = py_find(content, masks, lo, hi)
        assert starts == want, (case, content, bytes(needle), ignore_case, wild, lo, hi)
        assert any_ == int(any(want)), case
        if not ignore_case and not wild:
            by_find = [int(content.find(bytes(needle), p, p + m) == p) for p in range(lo, hi)]
            assert starts == by_find, case
        if ignore_case and not wild:
            by_find = [int(content.lower().find(bytes(needle).lower(), p, p + m) == p) for p in range(lo, hi)]
            assert starts == by_find, case
        hits += any_
    assert 40 < hits < 180  # both answers occur often


# ------------------------------------------------------------------ the needle-length limits
@pytest.mark.parametrize("m", nl.LENGTHS)
def test_plain_find_at_the_length_limits(m):
    """fr_plain_find against py_starts on needle_limits.TEXT: the needle of m characters at the
    last start that fits, as it is, case-insensitive, with wildcards and absent, over ranges that
    cut through that start; the text holds the needle and its near miss where its period says;
    and each of the 2 m selectors is read"""
    occ = nl.check_plain(F.plain_find, m)
    want, near = nl.known_starts(m)
    assert occ == want and len(nl.TEXT) - m in occ
    for p in near:
        assert p not in occ and nl.TEXT[p:p + m - 1] == nl.needle(m)[:-1]
    assert near or m > nl.DEVIANT + 1
    nl.check_every_test_counts(F.plain_find, m)


@pytest.mark.parametrize("m", nl.LENGTHS)
@pytest.mark.parametrize("starts", [False, True])
def test_schedule_at_the_length_limits(m, starts):
    """fr_schedule_find's jobs per level and level count from balanced_chunks(2 m) and or_tree;
    the sign gates' offsets; and every start's selector jobs carry the indices range(2 m), on
    the content blocks of character p + i"""
    n = len(nl.TEXT)
    for lo, hi in ((0, n), (n - m - 1, n - m + 1), (n - m, n), (n - m + 1, n)):
        S = F.schedule_find(n, m, lo, hi, starts=starts)
        fit = len(range(lo, min(hi, n - m + 1)))
        lvl1 = nl.check_levels(S, m, fit, starts, clear=False)
        assert len(S.parts) == (hi - lo if starts else 1)
        assert [p[0] >= 0 for p in S.parts] == ([True] * fit + [False] * (hi - lo - fit) if starts else [fit > 0])
        for at, j in enumerate(lvl1):
            p, t = lo + at // (2 * m), at % (2 * m)
            assert (j.kind, j.n_out, j.n_in, j.offset) == (F.JOB_ACC, 1, 2, 0)
            assert struct.unpack("<I", bytes(j.lut[0][:4]))[0] == t and not any(j.lut[0][4:])
            assert (j.in_ref[0], j.in_w[0]) == (content_ref(p + t // 2, 2 * (t % 2) + 1), 4)
            assert (j.in_ref[1], j.in_w[1]) == (content_ref(p + t // 2, 2 * (t % 2)), 1)
        assert {struct.unpack("<I", bytes(j.lut[0][:4]))[0] for j in lvl1} == (set(range(2 * m)) if fit else set())


def test_the_device_texts_hold_what_they_claim():
    """the slices tests/test_needle_limits_gpu.py runs: each a slice of TEXT with its 0x00 and
    bytes >= 0x80, the needle at the last start that fits (and where the comments say), the near
    miss at m = 8 and 16, two and three starts at m = 64; the three evaluators agree on them"""
    want = {8: ([0, 16], 8), 16: ([16], 0), 17: ([8], None), 64: ([2], None)}
    for m, text in list(nl.DEVICE_TEXT.items()) + [(64, nl.TEXT_65)]:
        assert text in nl.TEXT and len(text) <= 80 and text.count(0) == 1 and max(text) >= 0x80
        for evaluator in (F.plain_find, F.plain_find_clear, F.plain_scan_clear):
            occ = nl.check_plain(evaluator, m, text)
        occ_want, near = want[m] if text is not nl.TEXT_65 else ([1], None)
        assert occ == occ_want and occ[-1] == len(text) - m
        if near is not None:
            assert near not in occ and text[near:near + m - 1] == nl.needle(m, text)[:-1]
    assert sorted(nl.DEVICE_TEXT) == nl.LIMITS
    assert (len(nl.TEXT_65) - 63, len(nl.DEVICE_TEXT[64]) - 63) == (2, 3)
