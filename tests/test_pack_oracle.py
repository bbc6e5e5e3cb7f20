"""The packing keyswitch's independent restatement (oracle/pack_oracle.py: numpy and Python
integers, no code shared with the product) and the host code held to it, word for word.

Before this module pack_lwes / pack_lwes_mapped (pack_host in keys.cpp) were the reference of
every device pack test while sharing the ks_decompose template with the kernels, and were held
themselves only by algebra on trivial LWEs, by decryption and by a phase-error bound: a wrong
digit rule, a wrong sign at the negacyclic wrap or a mis-indexed key row made the same way on
both sides passed everything, and so did a word wrong once in 2^22 coefficients.

Here: (1) the directed operands of tests/gadget_edges.py are what they claim, and the
restatement's decomposition equals the oracle's C one at (3, 5) and (7, 3) on all of them;
(2) the restatement alone decrypts, through test_packed_results.negacyclic_phase and under that
file's 2^52 bound; (3) pack_lwes, pack_lwes_mapped and compress_packed equal the restatement on
real, edge and crafted operands at both points.  Every comparison is exact.

Wall time of the module, 30 tests: 25 s on a 16-thread build machine with nothing else running,
40 s measured on another; the host's own 33-row packs and the keys' limb planes are most of it.
Against the suite's ~5 minutes on the first machine that is a twelfth; the figure follows the
machine, the share less so.
"""
import ctypes as C

import numpy as np
import pytest

import fheregex as F
import gadget_edges as ge
import oracle_ffi as of
import pack_oracle as po
import test_packed_results as tp
import test_scan_clear_gpu as sc

U = np.uint64
POINTS = {"k1n2048": (1, 2048), "k2n1024": (2, 1024)}
PSEED = tp.PSEED
KINDS = ["real", "saturating", "mixed"]
N_EDGE = 33

_CLIENT, _KEY = {}, {}


def drop_key():
    """close the crafted context of the Key in use (a real key's context is its point's client)"""
    for ctx, _ in _KEY.values():
        if ctx not in _CLIENT.values():
            ctx.close()
    _KEY.clear()


@pytest.fixture(scope="module", autouse=True)
def released():
    """what the module caches (two clients with full packing keys, one Key with its f64 limb
    planes) is closed and dropped when the module ends, not when the session does"""
    yield
    drop_key()
    for ctx in _CLIENT.values():
        ctx.close()
    _CLIENT.clear()


def client(request, pid):
    """a host context with the client key and the real host-generated packing key, once per point"""
    if pid not in _CLIENT:
        ctx = tp.host(POINTS[pid], request.getfixturevalue("key_blob"))
        ctx.gen_packing_key(PSEED)
        _CLIENT[pid] = ctx
    return _CLIENT[pid]


def keyed(request, pid, kind):
    """(a host context holding the key `kind`, the restatement's Key of the same rows); the crafted
    keys sit in contexts of their own, loaded with load_packing_key.  One Key is kept at a time
    (its f64 limb planes are four times the rows)."""
    if (pid, kind) not in _KEY:
        drop_key()
        k, N = POINTS[pid]
        real = client(request, pid)
        blob = real.export_packing_key()
        if kind == "real":
            ctx, rows = real, np.frombuffer(blob, dtype="<u8", offset=48).reshape(3 * k * N, (k + 1) * N)
        else:
            rows = ge.crafted_key(kind, 3 * k * N, (k + 1) * N)
            ctx = F.Context(device=-1, params=F.default_params(k=k, N=N))
            ctx.load_packing_key(ge.packing_blob(blob[:48], rows))
        _KEY[pid, kind] = ctx, po.Key(rows, k, N)
    return _KEY[pid, kind]


def c_digits(x, B, L):
    d = (C.c_int32 * L)()
    of.lib().or_ks_decompose(int(x), B, L, d)
    return list(d)


# ------------------------------------------------------------------ the catalogue is what it claims
@pytest.mark.parametrize("B,L", [(3, 5), (7, 3)])
def test_edge_words_are_what_they_claim(B, L):
    h, s = 1 << (B - 1), 64 - B * L
    words = ge.edge_words(B, L)
    assert len(set(words.values())) == len(words) == 11 + 2 * L
    for name, x in ge.NAMED_WORDS[B, L].items():
        assert words[name] == x, name
    want = ge.expected_digits(B, L)
    assert set(want) <= set(words) and len(want) >= 9 + 2 * L
    rng = np.random.default_rng(B * L)
    xs = np.concatenate([np.array(list(words.values()), dtype=U), rng.integers(0, 2 ** 64, 4000, dtype=U)])
    got = po.decompose(xs, B, L)
    assert got.shape == (len(xs), L)
    for i, x in enumerate(xs):
        assert list(got[i]) == c_digits(x, B, L), hex(int(x))
    for i, name in enumerate(words):
        if name in want:
            assert list(got[i]) == want[name], name
    assert got.min() == -h and got.max() == h - 1
    # the digits put back together miss the word by the rounding alone (a half rounds up: the
    # error reaches -2^(s-1) and stays under +2^(s-1))
    err = (xs - po.recompose(got, B)).astype(np.int64)
    assert err.min() >= -(1 << (s - 1)) and err.max() <= (1 << (s - 1))
    assert err.min() == -(1 << (s - 1)) and err.max() == (1 << (s - 1)) - 1  # round-bit, under-round
    # Python integers, once more, on the catalogue: the closest multiple of 2^s mod 2^(B L)
    for i, x in enumerate(words.values()):
        v = ((x + (1 << (s - 1))) >> s) % (1 << (B * L))
        assert sum(int(d) << (B * (L - 1 - l)) for l, d in enumerate(got[i])) % (1 << (B * L)) == v


def test_crafted_words_and_rows_are_what_they_claim():
    for x, want in ge.NAMED_LIMBS.items():
        got = po.limbs(np.array([x], dtype=U))[0]
        assert list(got) == want, hex(x)
        assert sum(int(v) << (8 * l) for l, v in enumerate(got)) % 2 ** 64 == x
    xs = np.random.default_rng(8).integers(0, 2 ** 64, 4000, dtype=U)
    lm = po.limbs(xs)
    assert lm.min() == -128 and lm.max() == 127
    assert all(sum(int(v) << (8 * l) for l, v in enumerate(lm[i])) % 2 ** 64 == int(xs[i]) for i in range(len(xs)))
    # the keys: every word of the saturating key; the mixed key's cycle and its random eighth
    assert (ge.saturating_key(5, 7) == U(ge.SATURATING)).all()
    mk = ge.mixed_key(16, 24, 1)
    for r in range(16):
        for t in range(24):
            i = (r + 3 * t) % 8
            assert i == 7 or int(mk[r, t]) == ge.MIXED[i]
    assert len({int(v) for v in mk[(np.arange(16)[:, None] + 3 * np.arange(24)[None, :]) % 8 == 7]}) == 48
    assert np.array_equal(mk, ge.mixed_key(16, 24, 1)) and not np.array_equal(mk, ge.mixed_key(16, 24, 2))
    # the limb sums the source's exactness bounds speak of, reached by all-low against the saturating key
    assert 64 * 128 * 6144 == 50_331_648 < 2 ** 26 and 4 * 128 * 10240 == 5_242_880 < 2 ** 31
    # the rows
    for (B, L), big in (((7, 3), 2048), ((3, 5), 2048)):
        words = ge.edge_words(B, L)
        cat = list(words.values())
        names, rows = ge.lwe_rows(B, L, big, 97, 3)
        assert rows.shape == (97, big + 1) and len(names) == 97
        assert names[:3] == ["all-low", "catalogue", "all-top"] and names[-1] == "ends"
        assert set(words) | {"trivial-%d" % i for i in range(6)} | {"random", "catalogue", "ends"} == set(names)
        assert (po.decompose(rows[0, :big], B, L) == -(1 << (B - 1))).all()
        assert [int(v) for v in rows[1, :2 * len(cat)]] == cat + cat
        for name, x in words.items():
            assert (rows[names.index(name), :big] == U(x)).all(), name
        e = rows[-1, :big]
        assert [int(v) for v in e[:16]] == (cat + cat)[:16] and [int(v) for v in e[-16:]] == (cat[::-1] + cat[::-1])[:16]
        assert not e[16:-16].any()
        for i, (body, v) in enumerate(ge.ROUND16_EDGES):
            row = rows[names.index("trivial-%d" % i)]
            assert not row[:big].any() and int(row[big]) == body and int(po.round16(row[big:])[0]) == v
        for n in (1, 2, 3, 4, 33):
            nm, rw = ge.lwe_rows(B, L, big, n, 3)
            assert len(nm) == n == len(rw) and nm[0] == "all-low" and (n < 4 or nm[-1] == "ends")
    rows, vals = ge.trivial_rows(2048, 9)
    assert vals == [0, 0xFFFF, 1, 0, 0x8000, 0, 0, 0xFFFF, 1] and list(po.round16(rows[:, -1])) == vals


# ------------------------------------------------------------------ the restatement alone is right
def test_gemm_entries_in_python_integers(request):
    """Key.times against plain integer sums on sampled entries, with the largest operand"""
    _, key = keyed(request, "k1n2048", "mixed")
    _, rows = ge.lwe_rows(7, 3, 2048, 4, 5)
    D = po.digit_rows(rows, np.ones(4, dtype=np.int64), 1, 2048)
    assert (D[0] == -64).all()
    got = key.times(D)
    for r, col in ((0, 0), (0, 4095), (1, 7), (1, 2048), (3, 2047), (3, 3000)):
        assert int(got[r, col]) == key.entry(D[r], col), (r, col)
    # ... and numpy's own wrapping integer product on one row
    assert np.array_equal(got[1], D[1].astype(np.int64).astype(U) @ key.rows)


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("pid", list(POINTS))
def test_restatement_decrypts(request, pid, n):
    """fresh encryptions, a negated row and a constant through pack_oracle.pack alone; the phase
    is taken by negacyclic_phase, not by the library"""
    k, N = POINTS[pid]
    ctx, key = keyed(request, pid, "real")
    rng = np.random.default_rng(500 + n)
    bits = rng.integers(0, 2, n).astype(np.int64)
    lwes = ctx.encrypt_blocks(bits.astype(np.uint8), seed=91).reshape(n, -1)
    w, off = np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    want = bits.copy()
    if n >= 3:
        w[1], off[1], want[1] = -1, 2, 1 - bits[1]  # 1 - x
        w[2], off[2], want[2] = 0, 2, 1             # the constant 1, its LWE unread
    words = po.pack(key.rows, lwes, w, off, k, N) if n == 1 else po.pack(key, lwes, w, off)
    assert words.shape == ((k + 1) * N,)
    ph = tp.signed(tp.negacyclic_phase(words, tp.s_big(ctx), k, N))
    err = ph[:n] - (want << tp.DELTA_LOG)
    print("%s n=%d: largest error 2^%.2f" % (pid, n, np.log2(max(1, np.abs(err).max()))))
    assert np.abs(err).max() < 2 ** 52
    assert np.abs(ph[n:]).max() < 2 ** 52  # coefficients past n carry the key's noise only
    if n >= 3:  # a constant has no digit: its row of G is its body alone
        g = po.pack_rows(key, lwes, w, off)[2]
        assert int(g[k * N]) == 1 << tp.DELTA_LOG and np.count_nonzero(g) == 1


# ------------------------------------------------------------------ the host equals the restatement
def affine(n):
    """weights and offsets over the row count: a NOT's (-1, 2), constants, small multiples"""
    w = [(1, -1, 0, 2, -3)[r % 5] for r in range(n)]
    off = [(0, 2, 2, 1, -1)[r % 5] for r in range(n)]
    return w, off


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pid", list(POINTS))
def test_pack_lwes_equals_restatement(request, pid, kind):
    k, N = POINTS[pid]
    ctx, key = keyed(request, pid, kind)
    _, edge = ge.lwe_rows(7, 3, k * N, N_EDGE, 11)
    sets = [("edge", edge)]
    if kind == "real":
        bits = np.random.default_rng(3).integers(0, 2, N_EDGE).astype(np.uint8)
        real = client(request, pid).encrypt_blocks(bits, seed=17).reshape(N_EDGE, -1)
        sets += [("real", real), ("one", real[:1]), ("one-edge", edge[:1])]
    for name, lwes in sets:
        n = len(lwes)
        got, want = ctx.pack_lwes(lwes), po.pack(key, lwes)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        w, off = affine(n)
        got, want = ctx.pack_lwes(lwes, w, off), po.pack(key, lwes, w, off)
        assert np.array_equal(got, want), (name, "affine", int((got != want).sum()))
    # constants alone: no LWE is read
    assert np.array_equal(ctx.pack_lwes(None, [0, 0, 0], [2, 0, -1], n=3), po.pack(key, None, [0, 0, 0], [2, 0, -1], n=3))


@pytest.mark.parametrize("shape", ["1x3", "3x33-gaps", "33x65"])
@pytest.mark.parametrize("kind", ["real", "mixed"])
@pytest.mark.parametrize("pid", list(POINTS))
def test_pack_lwes_mapped_equals_restatement(request, pid, kind, shape):
    k, N = POINTS[pid]
    ctx, key = keyed(request, pid, kind)
    R, map_ = sc.shapes(N)[shape]
    _, lwes = ge.lwe_rows(7, 3, k * N, R, 13)
    got, want = ctx.pack_lwes_mapped(lwes, map_), po.pack_mapped(key, lwes, map_)
    assert np.array_equal(got, want), int((got != want).sum())
    w, off = affine(R)
    if R >= 3:
        w[0] = 1  # (every row is read by some start; a constant row stays among them)
    got, want = ctx.pack_lwes_mapped(lwes, map_, w, off), po.pack_mapped(key, lwes, map_, w, off)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("pid", list(POINTS))
def test_compress_equals_round16(request, pid, n):
    """trivial rows pack to their bodies, and the bodies are the rounding's edges"""
    k, N = POINTS[pid]
    ctx, key = keyed(request, pid, "real")
    lwes, vals = ge.trivial_rows(k * N, n)
    words = po.pack(key, lwes)
    assert not words[:k * N].any() and np.array_equal(words[k * N:k * N + n], lwes[:, -1]) and not words[k * N + n:].any()
    assert np.array_equal(ctx.pack_lwes(lwes), words)
    sent = np.frombuffer(ctx.compress_packed(words, n), dtype="<u2", offset=32)
    assert np.array_equal(sent, po.round16(words[:k * N + n]))
    assert list(sent[k * N:]) == vals
    # ... and on a real pack's words, every sent coefficient
    _, edge = ge.lwe_rows(7, 3, k * N, n, 19)
    words = po.pack(key, edge)
    sent = np.frombuffer(ctx.compress_packed(words, n), dtype="<u2", offset=32)
    assert np.array_equal(sent, po.round16(words[:k * N + n]))
