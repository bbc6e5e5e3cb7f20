"""ORACLE -- TEST INFRASTRUCTURE ONLY: the packing keyswitch and the compact rounding restated
in numpy and Python integers.  Imports neither fheregex nor libfheregex and holds no key
generation: the key rows come in as an array.

    G[r] = (0, .., 0, off[r] 2^58 + w[r] b_r) - D[r] x PKSK     pack_rows
    out  = sum_j X^j G[map[j]]  mod X^N + 1, per polynomial      rotate_sum

D[r] holds the signed (2^7, 3) digits of w[r] a_r mod 2^64, most significant level first; PKSK
has 3 kN rows of (k+1) N words, row 3 i + l under digit l of coefficient i.

Nothing here is shaped like the product's code.  The digits come from one offset addition and
plain bit fields, not from a carry chain: v = sum_l d_l 2^(B l) (mod 2^(B L)) with every d_l in
[-h, h) holds exactly when v + sum_l h 2^(B l) has the bit fields d_l + h.  The balanced byte
limbs are the same identity at B = 8.  The product D x PKSK is four f64 GEMMs over the key's
16-bit limbs, each partial sum at most 64 * 65535 * 6144 < 2^35 and so exact in f64, recombined
mod 2^64 (tests/test_packed_results.py's negacyclic_phase is the precedent).  The rotation
places every row in a line of 2 N coefficients and folds the upper half back with a minus sign.
"""
from __future__ import annotations

import numpy as np

U = np.uint64
PK_BASE_LOG, PK_LEVELS = 7, 3
HALF_DELTA_LOG = 58  # an offset counts in units of Delta / 2 = 2^58
M64 = (1 << 64) - 1


def decompose(words, B: int, L: int) -> np.ndarray:
    """signed digits of the words' closest multiples of 2^(64 - B L), wrapped mod 2^(B L): shape
    words.shape + (L,), most significant level first, every digit in [-2^(B-1), 2^(B-1))"""
    a = np.asarray(words, dtype=U)
    bits, h = B * L, 1 << (B - 1)
    s = 64 - bits
    assert 0 < s and B < 32
    v = (a + U(1 << (s - 1))) >> U(s)  # the addition wraps mod 2^64: the top word rounds up to 0
    shifted = (v + U(sum(h << (B * l) for l in range(L)))) & U((1 << bits) - 1)
    out = np.empty(a.shape + (L,), dtype=np.int32)
    for l in range(L):  # level l has weight 2^(64 - B (l + 1))
        field = (shifted >> U(B * (L - 1 - l))) & U((1 << B) - 1)
        out[..., l] = field.astype(np.int32) - h
    return out


def recompose(digits, B: int) -> np.ndarray:
    """sum_l d_l 2^(64 - B (l + 1)) mod 2^64"""
    d = np.asarray(digits)
    acc = np.zeros(d.shape[:-1], dtype=U)
    for l in range(d.shape[-1]):
        acc += d[..., l].astype(np.int64).astype(U) << U(64 - B * (l + 1))
    return acc


def limbs(words) -> np.ndarray:
    """the 8 balanced byte limbs, least significant first: words = sum_l limb_l 256^l (mod 2^64),
    every limb in [-128, 128)"""
    x = np.asarray(words, dtype=U) + U(0x8080808080808080)
    out = np.empty(x.shape + (8,), dtype=np.int32)
    for l in range(8):
        out[..., l] = ((x >> U(8 * l)) & U(0xFF)).astype(np.int32) - 128
    return out


def round16(words) -> np.ndarray:
    """the compact reply's rule: ((x + 2^47) >> 48) mod 2^16 (uint64 arithmetic wraps mod 2^64)"""
    return ((np.asarray(words, dtype=U) + U(1 << 47)) >> U(48)).astype(np.uint16)


class Key:
    """a packing key's rows (3 kN, (k+1) N) and, formed at the first product and kept, their four
    planes of 16-bit limbs as f64 (four times the rows' size; drop the Key to free them)"""

    def __init__(self, rows, k: int, N: int):
        self.k, self.N = k, N
        self.rows = np.asarray(rows, dtype=U).reshape(PK_LEVELS * k * N, (k + 1) * N)
        self._planes = None

    def planes(self):
        if self._planes is None:
            self._planes = [((self.rows >> U(16 * q)) & U(0xFFFF)).astype(np.float64) for q in range(4)]
        return self._planes

    def times(self, D) -> np.ndarray:
        """D x rows mod 2^64 for small signed D (|d| <= 64): (len(D), (k+1) N) words"""
        Df = np.asarray(D, dtype=np.float64)
        assert Df.shape[1] == self.rows.shape[0] and np.abs(Df).max(initial=0) <= 64
        acc = np.zeros((Df.shape[0], self.rows.shape[1]), dtype=U)
        for q, plane in enumerate(self.planes()):
            acc += (Df @ plane).astype(np.int64).astype(U) << U(16 * q)
        return acc

    def entry(self, d_row, col: int) -> int:
        """one word of d_row x rows in Python integers (the spot check of `times`)"""
        return sum(int(d) * int(x) for d, x in zip(d_row, self.rows[:, col]) if d) & M64


def _affine(n, w, off):
    w = np.ones(n, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    off = np.zeros(n, dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)
    assert w.shape == off.shape == (n,)
    return w, off


def digit_rows(lwes, w, k: int, N: int) -> np.ndarray:
    """D: row r holds the digits of w[r] a_r mod 2^64, coefficient-major (column 3 i + l); a row
    with w[r] = 0 is not read and has no digit"""
    big = k * N
    D = np.zeros((len(w), PK_LEVELS * big), dtype=np.int32)
    for r in np.flatnonzero(w):
        a = np.asarray(lwes[r][:big], dtype=U) * U(int(w[r]) & M64)
        D[r] = decompose(a, PK_BASE_LOG, PK_LEVELS).reshape(-1)
    return D


def as_key(pksk, k=None, N=None) -> Key:
    """a Key as it is (its planes cached); an array of rows wrapped for this call"""
    if isinstance(pksk, Key):
        assert (k is None or k == pksk.k) and (N is None or N == pksk.N)
        return pksk
    return Key(pksk, k, N)


def pack_rows(pksk, lwes, w=None, off=None, k=None, N=None, n_rows: int | None = None) -> np.ndarray:
    """G: one GLWE of (k+1) N words per boolean off[r] 2^58 + w[r] lwes[r]; pksk is a Key or the
    rows as an array (then k and N are needed); lwes may be None where every w is 0"""
    key = as_key(pksk, k, N)
    k, N = key.k, key.N
    big = k * N
    if lwes is not None:
        lwes = np.asarray(lwes, dtype=U).reshape(-1, big + 1)
        n_rows = len(lwes)
    w, off = _affine(n_rows, w, off)
    assert lwes is not None or not w.any()
    G = U(0) - key.times(digit_rows(lwes, w, k, N))
    for r in range(n_rows):
        body = (int(off[r]) << HALF_DELTA_LOG) + (int(w[r]) * int(lwes[r][big]) if w[r] else 0)
        G[r, big:big + 1] += U(body & M64)  # (an array add wraps silently)
    return G


def rotate_sum(G, n: int, N: int, map=None) -> np.ndarray:
    """sum_j X^j G[map[j]] over Z_2^64[X] / (X^N + 1), polynomial by polynomial, for the starts
    j < n; map None reads row j, map[j] < 0 contributes nothing"""
    G = np.asarray(G, dtype=U)
    polys = G.shape[1] // N
    assert G.shape[1] == polys * N and 1 <= n <= N
    line = np.zeros((polys, 2 * N), dtype=U)  # X^j G placed without reduction
    for j in range(n):
        r = j if map is None else int(map[j])
        if r >= 0:
            line[:, j:j + N] += G[r].reshape(polys, N)
    return (line[:, :N] - line[:, N:]).reshape(-1)  # X^N = -1


def pack(pksk, lwes, w=None, off=None, k=None, N=None, n: int | None = None) -> np.ndarray:
    """the (k+1) N words of the packed GLWE of n booleans"""
    key = as_key(pksk, k, N)
    G = pack_rows(key, lwes, w, off, n_rows=n)
    return rotate_sum(G, len(G), key.N)


def pack_mapped(pksk, lwes, map, w=None, off=None, k=None, N=None, n_rows: int | None = None) -> np.ndarray:
    """pack where start j reads row map[j] of the n_rows booleans"""
    key = as_key(pksk, k, N)
    G = pack_rows(key, lwes, w, off, n_rows=n_rows)
    assert all(int(m) < len(G) for m in map)
    return rotate_sum(G, len(map), key.N, map)
