"""Shared by tests/test_byte_needle.py and tests/test_byte_needle_gpu.py: the byte-table
extract-sum restated in numpy, the direct Python search over 256-bit sets, and the needles the
device tests run."""
import numpy as np

import fheregex as F

U = np.uint64
K = bytes((37 * i + 11) & 0xFF for i in range(32))  # a fixed 256-bit generator key
POINTS = {"k1n2048": (1, 2048), "k2n1024": (2, 1024)}
FRESH_BOUND = 2 ** 16  # a fresh GLWE coefficient's error (tests/test_private_needle.py: 12 sigma at k = 1)


def tpg(N):
    """tables per selector"""
    return N // 256


def coefficient(N, i, b):
    """(selector, coefficient) of byte b of table i"""
    return i // tpg(N), (i % tpg(N)) * 256 + b


def extract_sum_bytes(sel, content, terms):
    """out[c N + t] = sum over (i, pos, 0) of (t <= j ? A_{g,c}[j - t] : -A_{g,c}[N + j - t]),
    out[k N] = sum of B_g[j], with g = i / (N/256) and j = (i % (N/256)) 256 + content[pos]; sel is
    [selector][k + 1][N] u64.  Wrapping u64."""
    k, N = sel.shape[1] - 1, sel.shape[2]
    out = np.zeros(k * N + 1, dtype=U)
    t = np.arange(N)
    with np.errstate(over="ignore"):
        for i, pos, zero in terms:
            assert zero == 0
            g, j = coefficient(N, i, content[pos])
            for c in range(k):
                a = sel[g, c][(j - t) % N]
                out[c * N:(c + 1) * N] += np.where(t <= j, a, U(0) - a)
            out[k * N] += sel[g, k, j]
    return out


def table_poly(N, tables, g):
    """the phase selector g of a byte-table needle encrypts: T_i[b] 2^59 at (i % TPG) 256 + b, 0
    past the last table"""
    out = np.zeros(N, dtype=U)
    for s in range(tpg(N)):
        i = g * tpg(N) + s
        if i < len(tables):
            out[s * 256:(s + 1) * 256] = [((tables[i] >> b) & 1) << 59 for b in range(256)]
    return out


def py_find(content: bytes, tables, lo, hi):
    """the search itself: start p matches when every byte of its window is in its position's set"""
    m = len(tables)
    return [int(p + m <= len(content) and all((tables[i] >> content[p + i]) & 1 for i in range(m)))
            for p in range(lo, hi)]


def is_product(t: int) -> bool:
    """a 256-bit set that is lo_set x hi_set for a set of low and a set of high nibbles"""
    lo = {b & 15 for b in range(256) if (t >> b) & 1}
    hi = {b >> 4 for b in range(256) if (t >> b) & 1}
    return all(((t >> b) & 1) == int((b & 15) in lo and (b >> 4) in hi) for b in range(256))


def product_masks(t: int):
    """(lo_mask, hi_mask) of a product class"""
    assert is_product(t)
    lo = sum(1 << v for v in {b & 15 for b in range(256) if (t >> b) & 1})
    hi = sum(1 << v for v in {b >> 4 for b in range(256) if (t >> b) & 1})
    return lo, hi


# ------------------------------------------------------------------ the device tests' needles
# 40 bytes; "Id 4071" recurs, digits, letters of both cases, an x, a space, a byte >= 0x80
TEXT = b"Id 4071;ex 9a_Z\xe9 x7 Id 4071,id 40x1 q=8."
assert len(TEXT) == 40
# the items the issue names, cycled: literals, [0-9], [^x], . and \w
ITEMS = ["I", "d", " ", "[0-9]", "[0-9]", "[^x]", r"\w", ".", "[0-9]", r"\w", ";", "[^x]", "e", ".", " ", "[0-9]", "."]


def text_for(m):
    """40 bytes, or 80 for m = 64"""
    return TEXT if m <= 40 else TEXT + TEXT[::-1]


def pattern(m, at=0):
    """a pattern of m items that matches text_for(m) at `at`: the cycled items where they accept
    the byte there, else the byte's own literal as \\xHH"""
    text = text_for(m)
    out = []
    for i in range(m):
        item = ITEMS[i % len(ITEMS)]
        if not (F.needle_tables(item)[0] >> text[at + i]) & 1:
            item = "\\x%02x" % text[at + i]
        out.append(item)
    return "".join(out)
