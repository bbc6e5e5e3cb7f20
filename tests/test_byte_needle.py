"""Byte-table needles, host side (include/fheregex.h): needle_tables' grammar, the blob
"FRNEEDB1", the phases its selectors encrypt, the sample extract at any coefficient restated in
numpy, the lowering (fr_schedule_find_clear_bytes / fr_schedule_scan_clear_bytes) and its
plaintext evaluation.  No device: the kernel and the finds are tests/test_byte_needle_gpu.py.

The mask words are pinned to the ChaCha20 written out in tests/test_private_needle.py: stream 13
under the public mask key M = words 0..7 of block 0 of stream 8 under the generator key K."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import byte_needle_cases as bc
import fheregex as F
import oracle_ffi as of
from test_find_clear import or_tree
from test_private_needle import chacha_block, stream_u64

U = np.uint64
K = bc.K
HEADER = 64
STREAM_MASK_KEY, STREAM_NEEDLE_MASK, STREAM_NEEDLE_BYTES_MASK = 8, 11, 13
ALL = (1 << 256) - 1


def S(*items):
    """the 256-bit set of bytes, characters and (lo, hi) ranges written out"""
    t = 0
    for it in items:
        if isinstance(it, tuple):
            for b in range(ord(it[0]), ord(it[1]) + 1):
                t |= 1 << b
        else:
            t |= 1 << (it if isinstance(it, int) else ord(it))
    return t


DIGITS, UPPER, LOWER = S(("0", "9")), S(("A", "Z")), S(("a", "z"))
WORD = DIGITS | UPPER | LOWER | S("_")
SPACE = S(" ", "\t", "\n", "\r", "\f", "\v")


# ------------------------------------------------------------------ grammar
def test_needle_tables_by_hand():
    T = F.needle_tables
    assert T("a") == [S("a")]
    assert T(".") == [ALL]
    assert T("[0-9]") == [DIGITS]
    assert T("[^a]") == [ALL & ~S("a")]
    assert T(r"[a\-z]") == [S("a", "-", "z")]
    assert T(r"\d\W") == [DIGITS, ALL & ~WORD]
    assert T(r"\x00\xff") == [1, 1 << 255] == T(b"\\x00\\xff")
    assert T("[]-]") == [S("]", "-")]  # a ']' placed first and a '-' placed last are literals
    assert T("[-a]") == [S("-", "a")] and T("[a-]") == [S("a", "-")]
    assert T("[^]]") == [ALL & ~S("]")]
    assert T("[^^]") == [ALL & ~S("^")] and T("[a^]") == [S("a", "^")]
    assert T(r"[\d_a-c]") == [DIGITS | S("_", "a", "b", "c")]
    assert T(r"[\x41-\x43]") == [S("A", "B", "C")]
    assert T(r"\s\S\D\w") == [SPACE, ALL & ~SPACE, ALL & ~DIGITS, WORD]
    assert T(r"[^ \t]") == [ALL & ~S(" ", "\t")]
    assert T(r"\.\*\[\\\$") == [S("."), S("*"), S("["), S("\\"), S("$")]
    assert T("[0-9a-fA-F]") == [DIGITS | S(("a", "f")) | S(("A", "F"))]
    assert T(b"\x00\xe9") == [1, 1 << 0xE9] == T("\x00\xe9")  # every byte is a literal, 0x00 and >= 0x80 too
    assert T("a.[0-9]") == [S("a"), ALL, DIGITS]  # one character per item
    assert len(T("a" * 64)) == 64


def test_needle_tables_ignore_case():
    T = F.needle_tables
    assert T("a", ignore_case=True) == T("A", ignore_case=True) == [S("a", "A")]
    assert T("[a-c]", ignore_case=True) == [S(("a", "c")) | S(("A", "C"))]
    assert T("[^a]", ignore_case=True) == [ALL & ~S("a", "A")]  # folded before the class is negated
    assert T("1\\[", ignore_case=True) == T("1\\[") == [S("1"), S("[")]  # no letter
    assert T("@`", ignore_case=True) == [S("@"), S("`")]  # the letters' neighbours stay single
    assert T(r"\x41\w", ignore_case=True) == [S("a", "A"), WORD]


@pytest.mark.parametrize("bad", [
    "a*", "a+", "a?", "a|b", "(a)", "a)", "a{2}", "a}", "^a", "a$", "[]", "[^]", "[a", "a]", "[^\\x00-\\xff]",
    "", "a" * 65, ".[0-9]" * 33, "a\\", "\\q", "\\x4", "\\xg0", "[z-a]", "[a-\\d]", "Ā", "[\\", "\\1",
])
def test_needle_tables_refusals(bad):
    with pytest.raises(ValueError):
        F.needle_tables(bad)


def test_refusals_name_the_character():
    for bad, ch in (("ab*", "*"), ("a(b", "("), ("^a", "^"), ("ab$", "$"), ("a{3}", "{")):
        with pytest.raises(ValueError, match="needle pattern") as e:
            F.needle_tables(bad)
        assert repr(ch) in str(e.value), (bad, str(e.value))


# ------------------------------------------------------------------ blob
class Setup:
    def __init__(self, pid, key_blob):
        self.k, self.N = bc.POINTS[pid]
        self.tpg = bc.tpg(self.N)
        self.p = F.default_params(k=self.k, N=self.N, ring=F.RING_FFT)
        self.client = F.Context(device=-1, params=self.p)
        if self.k == 1:
            self.client.load_client_key(key_blob)  # the fixture key
        else:
            self.client.gen_client_key(7)
        self.server = F.Context(device=-1, params=self.p)  # never sees a client key


@pytest.fixture(scope="module", params=list(bc.POINTS))
def su(request, key_blob):
    return Setup(request.param, key_blob)


def rc_expand(ctx, blob):
    m = C.c_size_t()
    return F.lib().fr_expand_needle_bytes(ctx.h, bytes(blob), len(blob), None, 0, C.byref(m))


def test_size_formula_and_header(su):
    c = su.client
    for m in (1, su.tpg, su.tpg + 1, 64):
        G = -(-m * 256 // su.N)
        assert c.needle_bytes_size(m) == HEADER + 8 * G * su.N, m
        assert len(c.encrypt_needle_bytes([ALL] * m, K)) == c.needle_bytes_size(m)
    if su.k == 1:  # the issue's figures: 8 characters in 16 KB against the nibble form's 256 KB
        assert (c.needle_bytes_size(8), c.needle_size(8)) == (16448, 262208)
    tables = F.needle_tables("a[0-9].")
    blob = c.encrypt_needle_bytes(tables, K)
    magic, k, N, m = struct.unpack_from("<8siiQ", blob, 0)
    assert (magic, k, N, m) == (b"FRNEEDB1", su.k, su.N, 3) and blob[56:64] == bytes(8)
    assert blob[24:56] == struct.pack("<8I", *chacha_block(K, STREAM_MASK_KEY, 0)[:8])  # M = derive_mask_key(K)
    w = su.server.expand_needle_bytes(blob)
    G = -(-3 * 256 // su.N)
    assert w.shape == (G, su.k + 1, su.N)
    assert np.array_equal(np.frombuffer(blob, dtype="<u8", offset=HEADER).reshape(G, su.N), w[:, -1])
    # size query, a larger buffer, a smaller one
    flat = F._tables_bytes(tables)
    n = C.c_size_t()
    F._check(F.lib().fr_encrypt_needle_bytes_keyed(c.h, flat, 3, K, None, 0, C.byref(n)))
    assert n.value == len(blob)
    buf = C.create_string_buffer(b"\xA5" * (len(blob) + 16), len(blob) + 16)
    F._check(F.lib().fr_encrypt_needle_bytes_keyed(c.h, flat, 3, K, buf, len(blob) + 16, C.byref(n)))
    assert buf.raw[:len(blob)] == blob and buf.raw[len(blob):] == b"\xA5" * 16
    assert F.lib().fr_encrypt_needle_bytes_keyed(c.h, flat, 3, K, buf, len(blob) - 1, C.byref(n)) == F.ERR_INVALID


def test_seeds_and_the_mask_key(su):
    c = su.client
    tables = F.needle_tables("[a-z]b")
    assert c.encrypt_needle_bytes(tables, K) == c.encrypt_needle_bytes(tables, K)
    a5, a6 = c.encrypt_needle_bytes(tables, 5), c.encrypt_needle_bytes(tables, 6)
    assert a5 == c.encrypt_needle_bytes(tables, 5) != a6
    assert a5[24:56] != a6[24:56]
    assert (np.frombuffer(a5, dtype="<u8", offset=HEADER) != np.frombuffer(a6, dtype="<u8", offset=HEADER)).all()
    a, b = c.encrypt_needle_bytes(tables), c.encrypt_needle_bytes(tables)  # NULL key: the OS CSPRNG
    assert a[24:56] != b[24:56]
    # the mask key is the nibble needle's for the same generator key, the streams are not
    nib = c.encrypt_needle(F.needle_masks("ab"), K)
    byt = c.encrypt_needle_bytes(tables, K)
    assert nib[24:56] == byt[24:56]
    assert int(su.server.expand_needle(nib)[0, 0, 0]) != int(su.server.expand_needle_bytes(byt)[0, 0, 0])


def test_mask_words_depend_on_the_mask_key_alone(su):
    """mask word t of mask polynomial c of selector g = u64 number (g k + c) N + t of stream 13
    under M: not stream 11's, nothing of K's own stream, and the same for another needle's tables"""
    m = su.tpg + 1
    blob = su.client.encrypt_needle_bytes(F.needle_tables("[0-9]" * m), K)
    M = blob[24:56]
    assert M != K
    w = su.server.expand_needle_bytes(blob)
    k, N = su.k, su.N
    for g, cc, t in [(0, 0, 0), (0, 0, 7), (0, 0, 8), (0, k - 1, N - 1), (1, 0, 0), (1, k - 1, 5), (1, k - 1, N - 1)]:
        idx = (g * k + cc) * N + t
        assert int(w[g, cc, t]) == stream_u64(M, STREAM_NEEDLE_BYTES_MASK, idx), (g, cc, t)
        assert int(w[g, cc, t]) != stream_u64(M, STREAM_NEEDLE_MASK, idx)
        assert int(w[g, cc, t]) != stream_u64(K, STREAM_NEEDLE_BYTES_MASK, idx)
    other = su.server.expand_needle_bytes(su.client.encrypt_needle_bytes(F.needle_tables("x" * m), K))
    assert np.array_equal(other[:, :-1], w[:, :-1]) and (other[:, -1] != w[:, -1]).any()


def test_refusals(su):
    c, s = su.client, su.server
    blob = c.encrypt_needle_bytes(F.needle_tables("a."), K)
    assert rc_expand(s, blob) == F.FR_OK

    def put(off, fmt, v):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)

    bad = {
        "one byte short": blob[:-1],
        "one byte long": blob + bytes(1),
        "header only": blob[:HEADER],
        "shorter than the header": blob[:40],
        "magic": b"FRNEEDB0" + blob[8:],
        "the nibble needle's magic": b"FRNEEDL1" + blob[8:],
        "k": put(8, "<i", 3 - su.k),
        "N": put(12, "<i", su.N // 2),
        "m = 0": put(16, "<Q", 0),
        "m = 65": put(16, "<Q", 65),
        "m past the blob's selectors": put(16, "<Q", su.tpg + 1),
        "m = 2^61": put(16, "<Q", 2 ** 61),
        "pad": put(56, "<Q", 1),
    }
    for name, b in bad.items():
        assert rc_expand(s, b) == F.ERR_INVALID, name
    # a well-formed blob of 65 characters' length is refused by m alone
    long = put(16, "<Q", 65)[:HEADER] + bytes(8 * -(-65 * 256 // su.N) * su.N)
    assert rc_expand(s, long) == F.ERR_INVALID
    n = C.c_size_t()
    for m in (0, 65):
        assert F.lib().fr_needle_bytes_size(c.h, m, C.byref(n)) == F.ERR_INVALID
        assert F.lib().fr_encrypt_needle_bytes_keyed(c.h, bytes(32 * 65), m, K, None, 0, C.byref(n)) == F.ERR_INVALID
    # the nibble needle's entries refuse this blob, and these refuse the nibble needle's
    assert F.lib().fr_expand_needle(s.h, blob, len(blob), None, 0, C.byref(n)) == F.ERR_INVALID
    nib = c.encrypt_needle(F.needle_masks("a"), K)
    assert rc_expand(s, nib) == F.ERR_INVALID
    # too few words to expand into; a server needs no key, a client without one cannot encrypt
    words = np.zeros((su.k + 1) * su.N - 1, dtype=U)
    assert F.lib().fr_expand_needle_bytes(s.h, blob, len(blob), F._p(words), words.size, C.byref(n)) == F.ERR_INVALID
    assert F.lib().fr_encrypt_needle_bytes_keyed(s.h, bytes(32), 1, K, None, 0, C.byref(n)) == F.ERR_NO_KEY
    # a host-only context has no device to upload to; a blob of neither magic is still refused
    h = C.c_void_p()
    assert F.lib().fr_upload_needle(s.h, blob, len(blob), C.byref(h)) == F.ERR_NO_DEVICE
    for b in (b"FRNEEDX1" + blob[8:], b"FRNEEDB0" + blob[8:], b"FRNEED"):
        assert F.lib().fr_upload_needle(s.h, b, len(b), C.byref(h)) == F.ERR_INVALID
    assert F.lib().fr_upload_needle(s.h, blob[:-1], len(blob) - 1, C.byref(h)) == F.ERR_INVALID  # before the device


def test_rns_ring_refuses(key_blob):
    c = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_RNS))
    c.load_client_key(key_blob)
    n = C.c_size_t()
    assert F.lib().fr_encrypt_needle_bytes_keyed(c.h, bytes(32), 1, K, None, 0, C.byref(n)) == F.ERR_INVALID
    assert "FFT ring only" in F.lib().fr_last_error().decode()
    fft = F.Context(device=-1, params=F.default_params(k=1, N=2048, ring=F.RING_FFT))
    fft.load_client_key(key_blob)
    assert rc_expand(c, fft.encrypt_needle_bytes([1], K)) == F.ERR_INVALID


# ------------------------------------------------------------------ phases and extraction
class Phases:
    """an m = TPG + 1 needle of classes that are not product classes, its expanded selectors and
    the error of every coefficient of their phases under the client's GLWE key"""

    def __init__(self, pid, key_blob, fixture_key):
        self.k, self.N = bc.POINTS[pid]
        self.tpg = bc.tpg(self.N)
        self.ctx = F.Context(device=-1, params=F.default_params(k=self.k, N=self.N, ring=F.RING_FFT))
        self.ctx.load_client_key(key_blob)
        # (phases under the big key only: no server key is generated)
        self.O = of.Oracle(fixture_key, seed=42, k=self.k, N=self.N, with_bsk=False, ring=of.RING_FFT)
        items = ["[0-9]", r"\w", "[^x]", "a", ".", r"[\x00\xff]", "[a-z]", r"\s", "[0-9a-fA-F]"]
        self.tables = F.needle_tables("".join(items[i % len(items)] for i in range(self.tpg + 1)))
        self.sel = self.ctx.expand_needle_bytes(self.ctx.encrypt_needle_bytes(self.tables, K))
        self.err = np.stack([(self.ctx.packed_phase(self.sel[g].reshape(-1)) - bc.table_poly(self.N, self.tables, g))
                             .view(np.int64) for g in range(len(self.sel))])


@pytest.fixture(scope="module", params=list(bc.POINTS))
def ph(request, key_blob, fixture_key):
    return Phases(request.param, key_blob, fixture_key)


def test_phases_are_the_tables(ph):
    """coefficient (i % TPG) 256 + b of selector i / TPG is T_i[b] 2^59 for every b of every table,
    and the unused coefficients of the last selector are 0, all within a fresh coefficient's bound"""
    assert len(ph.tables) == ph.tpg + 1 and ph.sel.shape == (2, ph.k + 1, ph.N)
    assert not all(bc.is_product(t) for t in ph.tables)
    for i, t in enumerate(ph.tables):
        g, j0 = bc.coefficient(ph.N, i, 0)
        phase = ph.ctx.packed_phase(ph.sel[g].reshape(-1))[j0:j0 + 256]
        want = np.array([((t >> b) & 1) << 59 for b in range(256)], dtype=U)
        assert np.abs((phase - want).view(np.int64)).max() < bc.FRESH_BOUND, i
    unused = ph.ctx.packed_phase(ph.sel[1].reshape(-1))[256:]
    assert len(unused) == ph.N - 256 and np.abs(unused.view(np.int64)).max() < bc.FRESH_BOUND
    assert np.abs(ph.err).max() < bc.FRESH_BOUND and ph.err.any()  # and there is noise
    print("largest byte-table phase error: 2^%.1f" % np.log2(np.abs(ph.err).max()))


def test_extract_is_an_lwe_of_the_table_bit(ph):
    """the extracted LWE's phase under the flattened key is the table's bit times 2^59 plus exactly
    the error of that coefficient: j = 0, j = N - 1 and one j in every table slot"""
    N = ph.N
    probes = [(0, 0x00), (ph.tpg - 1, 0xFF), (ph.tpg, 0x41)] + [(s, (37 * s + 5) % 256) for s in range(ph.tpg)]
    assert bc.coefficient(N, 0, 0x00) == (0, 0) and bc.coefficient(N, ph.tpg - 1, 0xFF) == (0, N - 1)
    for i, b in probes:
        g, j = bc.coefficient(N, i, b)
        lwe = bc.extract_sum_bytes(ph.sel, bytes([0x33, b]), [(i, 1, 0)])
        want = U(((ph.tables[i] >> b) & 1) << 59)
        err = int((ph.O.phase(lwe) - want).view(np.int64)[0])
        assert err == int(ph.err[g, j]), (i, b)


def test_sum_of_sixteen_extracts(ph):
    """a 16-term sum over both selectors: the count times 2^59 plus exactly the sum of its terms'
    errors (extraction is linear)"""
    content = bytes([0x30, 0x78, 0x61, 0xFF, 0x00, 0x5F, 0x20, 0x39])
    terms = [((5 * i) % (ph.tpg + 1), i % 8, 0) for i in range(15)] + [(ph.tpg, 3, 0)]
    count = sum((ph.tables[i] >> content[pos]) & 1 for i, pos, _ in terms)
    assert 0 < count < 16 and {bc.coefficient(ph.N, i, 0)[0] for i, _, _ in terms} == {0, 1}
    lwe = bc.extract_sum_bytes(ph.sel, content, terms)
    err = int((ph.O.phase(lwe) - U(count << 59)).view(np.int64)[0])
    assert err == sum(int(ph.err[bc.coefficient(ph.N, i, content[pos])]) for i, pos, _ in terms)


# ------------------------------------------------------------------ schedule, from the formula
def chunk_lens(m):
    """balanced chunks of at most 16 of m tests, the longer ones first"""
    c = -(-m // 16)
    return [m // c + (1 if i < m % c else 0) for i in range(c)]


def test_rotation_totals_over_256_characters():
    n = 256
    s = F.schedule_find_clear_bytes(n, 3, starts=True)
    assert (len(s.jobs), len(s.level_off) - 1) == (254, 1)
    s = F.schedule_find_clear_bytes(n, 3)
    assert (len(s.jobs), len(s.level_off) - 1) == (254 + 16 + 1, 3) == (271, 3)
    # m = 16: one sign gate per start where the nibble form takes two chunk gates and an AND
    s = F.schedule_find_clear_bytes(n, 16, starts=True)
    assert (len(s.jobs), len(s.level_off) - 1) == (241, 1)
    assert all((j.kind, j.n_in, j.in_w[0], j.offset) == (F.JOB_SIGN, 1, 1, -31) for j in s.jobs)
    assert len(F.schedule_find_clear(n, 16, starts=True).jobs) == 3 * 241 == 723
    assert len(F.schedule_find_clear_bytes(n, 16).jobs) == 241 + or_tree(241)
    # m = 17: chunks of 9 and 8, then their AND
    s = F.schedule_find_clear_bytes(n, 17, starts=True)
    fit = n - 17 + 1
    assert chunk_lens(17) == [9, 8] and len(s.level_off) - 1 == 2
    lvl1, lvl2 = s.jobs[:s.level_off[1]], s.jobs[s.level_off[1]:]
    assert [j.offset for j in lvl1] == [-17, -15] * fit and all(j.n_in == 1 and j.in_w[0] == 1 for j in lvl1)
    assert len(lvl2) == fit and all((j.n_in, j.offset) == (2, -3) for j in lvl2)
    for p, j in enumerate(lvl2):
        assert [j.in_ref[0], j.in_ref[1]] == [lvl1[2 * p].out_gate[0], lvl1[2 * p + 1].out_gate[0]]
    # m = 64: four chunks of 16 and the AND, against the nibble form's eight and the AND
    s = F.schedule_find_clear_bytes(n, 64, starts=True)
    fit = n - 64 + 1
    assert chunk_lens(64) == [16] * 4 and len(s.jobs) == fit * 5 and len(s.level_off) - 1 == 2
    assert all(j.offset == -31 for j in s.jobs[:s.level_off[1]]) and s.level_off[1] == 4 * fit
    assert all((j.n_in, j.offset) == (4, -7) for j in s.jobs[s.level_off[1]:])
    assert len(F.schedule_find_clear(n, 64, starts=True).jobs) == fit * 9


@pytest.mark.parametrize("n_chars,m", [(16, 1), (16, 8), (40, 16), (40, 17), (5, 5), (4, 5)])
@pytest.mark.parametrize("starts", [False, True])
def test_schedule(n_chars, m, starts):
    s = F.schedule_find_clear_bytes(n_chars, m, starts=starts)
    fit = max(n_chars - m + 1, 0)
    assert all(j.kind == F.JOB_SIGN for j in s.jobs)
    if fit == 0:
        assert s.jobs == [] and s.parts == ([(-1, 0, 0)] * n_chars if starts else [(-1, 0, 0)])
        return
    chunks = chunk_lens(m)
    lvl1 = s.jobs[:s.level_off[1]]
    made = {j.out_gate[0] for j in s.jobs}
    assert len(lvl1) == len(chunks) * fit
    for i, j in enumerate(lvl1):  # each over one extract-sum, a program gate that no job makes
        assert (j.n_in, j.n_out, j.in_w[0], j.offset) == (1, 1, 1, 1 - 2 * chunks[i % len(chunks)])
        assert j.in_ref[0] >= 0 and j.in_ref[0] not in made
    assert len({j.in_ref[0] for j in lvl1}) == len(lvl1)
    and_levels = 1 if len(chunks) == 1 else 2
    ands = fit if len(chunks) > 1 else 0
    if starts:
        assert len(s.jobs) == len(lvl1) + ands and len(s.level_off) - 1 == and_levels
        assert [p[0] >= 0 for p in s.parts] == [True] * fit + [False] * (n_chars - fit)
    else:
        assert len(s.jobs) == len(lvl1) + ands + or_tree(fit) and len(s.parts) == 1


def test_window_program():
    """Dpad = 64 windows: 64 + 4 + 1 jobs; a window's terms read the compacted text at stride m,
    which the plaintext route checks; stride 1 (m = 1) is the find's, job for job"""
    for m in (3, 16):
        s = F.schedule_scan_clear_bytes(64, m)
        assert (len(s.jobs), len(s.level_off) - 1) == (64 + 4 + 1, 3)
        assert all(j.offset == 1 - 2 * m for j in s.jobs[:64])
        assert len(F.schedule_scan_clear_bytes(64, m, starts=True).jobs) == 64
    s = F.schedule_scan_clear_bytes(64, 17, starts=True)
    assert len(s.jobs) == 64 * 3 and [j.offset for j in s.jobs[:4]] == [-17, -15, -17, -15]

    def flat(s):
        return [(j.kind, j.n_in, j.n_out, j.offset, list(j.in_ref[:j.n_in]), list(j.in_w[:j.n_in]), j.out_gate[0])
                for j in s.jobs], s.level_off, s.parts

    for starts in (False, True):
        assert flat(F.schedule_scan_clear_bytes(64, 1, starts)) == flat(F.schedule_find_clear_bytes(64, 1, 0, 64, starts))


def test_schedule_bounds():
    nj, nl, ns = C.c_size_t(), C.c_size_t(), C.c_size_t()
    outs = (C.c_int32 * 3)()
    fn = F.lib().fr_schedule_find_clear_bytes
    for m in (0, 65):
        assert fn(16, m, 0, 16, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
        assert F.lib().fr_schedule_scan_clear_bytes(64, m, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1,
                                                    C.byref(ns)) == F.ERR_INVALID
    assert fn(16, 3, 5, 4, 0, None, 0, C.byref(nj), None, 0, C.byref(nl), outs, 1, C.byref(ns)) == F.ERR_INVALID
    any_ = C.c_int32()
    buf = (C.c_uint8 * 1)()
    for f in (F.lib().fr_plain_find_clear_bytes, F.lib().fr_plain_scan_clear_bytes):
        assert f(b"abc", 3, bytes(32), 0, 0, 1, buf, C.byref(any_)) == F.ERR_INVALID
        assert f(b"abc", 3, bytes(32 * 65), 65, 0, 1, buf, C.byref(any_)) == F.ERR_INVALID
        assert f(b"abc", 3, None, 1, 0, 1, buf, C.byref(any_)) == F.ERR_INVALID


# ------------------------------------------------------------------ plain evaluation
def random_class(rng, byte):
    """a set that holds `byte`, of one of several kinds; most are not product classes"""
    kind = rng.randrange(6)
    if kind == 0:
        return 1 << byte
    if kind == 1:
        return ALL
    if kind == 2:  # a range around the byte
        lo, hi = rng.randint(0, byte), rng.randint(byte, 255)
        return sum(1 << b for b in range(lo, hi + 1))
    if kind == 3:  # everything but another byte
        return ALL & ~(1 << ((byte + rng.randint(1, 255)) % 256))
    if kind == 4:  # a random half of the bytes
        return rng.getrandbits(256) | (1 << byte)
    return (DIGITS | S("_")) | (1 << byte)


def test_plain_against_python():
    """200 seeded cases over all byte values, random classes per position, every case with at
    least one class that is no product lo_set x hi_set; every start and the OR, by the find's
    route and by the scan's"""
    rng = random.Random(20261021)
    hits = 0
    for case in range(200):
        n, m = rng.randint(1, 40), min(rng.randint(1, 20), rng.randint(1, 20))
        alphabet = bytes(range(256)) if case % 2 else b"\x00a0A_\xe9\xff 9"
        content = bytes(rng.choice(alphabet) for _ in range(n))
        at = rng.randint(0, n - m) if m <= n and rng.random() < 0.7 else None
        window = content[at:at + m] if at is not None else bytes(rng.choice(alphabet) for _ in range(m))
        tables = [random_class(rng, b) for b in window]
        while all(bc.is_product(t) for t in tables):
            i = rng.randrange(m)
            tables[i] = ALL & ~(1 << ((window[i] + 1 + rng.randrange(255)) % 256))  # [^c]: never a product
        assert not all(bc.is_product(t) for t in tables), case
        lo = rng.randint(0, n // 2)
        hi = rng.randint((lo + n) // 2, n + 2)  # (past the end: starts that cannot fit)
        want = bc.py_find(content, tables, lo, hi)
        starts, any_ = F.plain_find_clear_bytes(content, tables, lo, hi)
        assert starts == want, (case, content, lo, hi)
        assert any_ == int(any(want)), case
        assert F.plain_scan_clear_bytes(content, tables, lo, hi) == (want, int(any(want))), case
        hits += any_
    assert 40 < hits < 190  # both answers occur often


def test_product_classes_equal_the_nibble_needle():
    rng = random.Random(7)
    for case in range(40):
        n, m = rng.randint(1, 30), rng.randint(1, 18)
        content = bytes(rng.choice(b"abAB\x00\xff?") for _ in range(n))
        needle = bytes(rng.choice(b"abAB\x00\xff?") for _ in range(m))
        ic = rng.random() < 0.5
        masks = F.needle_masks(needle, ic, "?")
        tables = [sum(1 << b for b in range(256) if (lo >> (b & 15)) & 1 and (hi >> (b >> 4)) & 1) for lo, hi in masks]
        assert all(bc.is_product(t) and bc.product_masks(t) == mk for t, mk in zip(tables, masks))
        assert F.plain_find_clear_bytes(content, tables) == F.plain_find_clear(content, masks), case
        assert F.plain_scan_clear_bytes(content, tables) == F.plain_scan_clear(content, masks), case


def test_the_device_tests_needles():
    """tests/test_byte_needle_gpu.py's patterns match where they are built to, and mix the items"""
    for m in (1, 8, 9, 16, 17, 64):
        text = bc.text_for(m)
        tables = F.needle_tables(bc.pattern(m))
        assert len(tables) == m and bc.py_find(text, tables, 0, len(text))[0] == 1
    assert sum(bc.py_find(bc.TEXT, F.needle_tables(bc.pattern(5)), 0, 40)) >= 2  # "Id 40" recurs
    assert not all(bc.is_product(t) for t in F.needle_tables(bc.pattern(8)))


# ------------------------------------------------------------------ header, symbols
NEW = ["fr_needle_bytes_size", "fr_encrypt_needle_bytes_keyed", "fr_expand_needle_bytes", "fr_needle_form",
       "fr_schedule_find_clear_bytes", "fr_schedule_scan_clear_bytes", "fr_plain_find_clear_bytes",
       "fr_plain_scan_clear_bytes"]


def test_header_and_symbols():
    syms = F.header_symbols()
    for name in NEW:
        assert name in syms, name
        assert hasattr(F.lib(), name), name
        assert name in F._SIGS, name
    assert (F.NEEDLE_NIBBLES, F.NEEDLE_BYTES) == (0, 1)


def test_needle_form_refuses_null():
    f = C.c_int32()
    assert F.lib().fr_needle_form(None, C.byref(f)) == F.ERR_INVALID
