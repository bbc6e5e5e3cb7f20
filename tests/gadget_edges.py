"""Directed operands for both keyswitches: edge mask words of a gadget (B, L), LWE rows built
from them, the compact rounding's edge bodies, and crafted keys (no GPU use, no test functions;
tests/gate_programs.py is the precedent).  tests/test_pack_oracle.py checks that every operand
is what it claims; tests/test_pack_oracle_gpu.py runs them on the device.

With h = 2^(B-1) and s = 64 - B L, a word's digits are those of its closest multiple of 2^s,
wrapped mod 2^(B L), every digit in [-h, h).  Fresh encryptions look uniform, and the words that
matter each have probability 2^-(B L) or less: the round-up that wraps to all-zero digits, the
carry that ripples through every level, all digits at -h.  Here each is a row of its own.

The crafted keys reach the exactness bounds keyswitch.hip states.  Every word of the saturating
key has the balanced byte limbs -128 x 8; under a row of all -h digits every i32 limb sum of the
GEMM is then h * 128 * KD / GZ: 50,331,648 for the packing key (h = 64, KD = 6144) in one K
slice, 5,242,880 for the LWE keyswitch key (h = 4, KD = 10240).  Random operands give sums near
sqrt(KD).  Keys are drawn at run time from a seed; none is a fixture.
"""
from __future__ import annotations

import numpy as np

U = np.uint64
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ edge mask words
def all_digits(B: int, L: int, d: int) -> int:
    """the word whose L digits are all d (no rounding bit below them)"""
    return sum(d << (64 - B * (l + 1)) for l in range(L)) & M64


def edge_words(B: int, L: int) -> dict:
    """name -> word"""
    h, s = 1 << (B - 1), 64 - B * L
    low, top = all_digits(B, L, -h), all_digits(B, L, h - 1)
    words = {
        "zero": 0,
        "ones": M64,                       # rounds up and wraps: digits all 0
        "msb": 1 << 63,                    # top digit -h, its carry dropped
        "all-low": low,                    # digits all -h: the largest operand of the GEMM
        "all-top": top,                    # digits all h - 1
        "all-top+round": top + (1 << (s - 1)),   # a carry through every level: all -h
        "all-top+below": top + (1 << s) - 1,     # the same from every bit under the gadget
        "round-bit": 1 << (s - 1),         # a lone rounding bit: lowest digit 1
        "under-round": (1 << (s - 1)) - 1,  # digits all 0
        "neg-all-low": -low & M64,         # what a handle negated with w = -1 makes of all-low
        "neg-all-top": -top & M64,
    }
    for l in range(L):
        words["plus-one-at-%d" % l] = 1 << (64 - B * (l + 1))
        words["minus-one-at-%d" % l] = -(1 << (64 - B * (l + 1))) & M64
    return words


# digit lists and words worked out by hand with Python integers, most significant level first
NAMED_DIGITS = {
    (7, 3): {"all-low": [-64] * 3, "all-top": [63] * 3, "neg-all-low": [-63, -63, -64], "neg-all-top": [-63] * 3},
    (3, 5): {"all-low": [-4] * 5, "all-top": [3] * 5},
}
NAMED_WORDS = {
    (7, 3): {"all-low": 0x7EFE000000000000, "all-top": 0x7EFDF80000000000},
    (3, 5): {"all-low": 0x6DB8000000000000, "all-top": 0x6DB6000000000000},
}


def expected_digits(B: int, L: int) -> dict:
    """name -> the digits every catalogue word must have, by construction"""
    h = 1 << (B - 1)
    want = {"zero": [0] * L, "ones": [0] * L, "msb": [-h] + [0] * (L - 1), "all-low": [-h] * L, "all-top": [h - 1] * L,
            "all-top+round": [-h] * L, "all-top+below": [-h] * L, "round-bit": [0] * (L - 1) + [1],
            "under-round": [0] * L}
    for l in range(L):
        want["plus-one-at-%d" % l] = [int(j == l) for j in range(L)]
        want["minus-one-at-%d" % l] = [-int(j == l) for j in range(L)]
    want.update(NAMED_DIGITS[B, L])
    return want


# ------------------------------------------------------------------ the compact rounding's edges
# body word -> the 16-bit value it is sent as
ROUND16_EDGES = [
    (0xFFFF800000000000, 0),       # the top value's half rounds up and wraps
    (0xFFFF7FFFFFFFFFFF, 0xFFFF),  # one under it stays
    (0x0000800000000000, 1),       # a half rounds up
    (0x00007FFFFFFFFFFF, 0),       # one under a half rounds down
    (0x7FFF800000000000, 0x8000),  # into the sign bit
    (M64, 0),
]


# ------------------------------------------------------------------ LWE rows
def lwe_rows(B: int, L: int, big: int, n: int, seed: int) -> tuple:
    """(names, (n, big + 1) words): n edge rows of big mask words and a body.

    Row 0 is all-low, row 1 cycles through the whole catalogue, row 2 (the one a test negates) is
    all-top; the last row (n >= 4) holds the catalogue in its first and last 16 coefficients and
    zeros between (a digit pass may write 16 coefficients per thread), so that the padding rows
    of a launch follow an edge row.  Between them: one row per remaining edge word, filled with
    it; trivial rows (zero mask) whose bodies are the ROUND16_EDGES; random rows."""
    rng = np.random.default_rng(seed)
    words = edge_words(B, L)
    cat = np.array(list(words.values()), dtype=U)
    rows, names = np.zeros((n, big + 1), dtype=U), []

    def put(name, mask, body=None):
        r = len(names)
        if r < n:
            rows[r, :big] = mask
            rows[r, big] = rng.integers(0, 2 ** 64, dtype=U) if body is None else U(body)
            names.append(name)

    last = n - 1 if n >= 4 else n  # the row kept for "ends"
    put("all-low", U(words["all-low"]))
    put("catalogue", np.resize(cat, big))
    put("all-top", U(words["all-top"]))
    for name, x in words.items():
        if name not in ("all-low", "all-top") and len(names) < last:
            put(name, U(x))
    for i, (body, _) in enumerate(ROUND16_EDGES):
        if len(names) < last:
            put("trivial-%d" % i, U(0), body)
    while len(names) < last:
        put("random", rng.integers(0, 2 ** 64, big, dtype=U))
    if n >= 4:
        ends = np.zeros(big, dtype=U)
        ends[:16], ends[-16:] = np.resize(cat, 16), np.resize(cat[::-1], 16)
        put("ends", ends)
    return names, rows


def trivial_rows(big: int, n: int) -> tuple:
    """(n rows of zero mask whose bodies cycle through ROUND16_EDGES, the n values they are sent as)"""
    rows = np.zeros((n, big + 1), dtype=U)
    vals = []
    for r in range(n):
        body, v = ROUND16_EDGES[r % len(ROUND16_EDGES)]
        rows[r, big] = U(body)
        vals.append(v)
    return rows, vals


# ------------------------------------------------------------------ crafted keys
SATURATING = 0x7F7F7F7F7F7F7F80  # limbs -128 x 8, a carry through all eight bytes
MIXED = [SATURATING,
         0x7F7F7F7F7F7F7F7F,     # limbs all 127
         0x8080808080808080,     # limbs -128, then -127 x 7
         0, M64, 1 << 63, 0x80]  # ... and, eighth, a seeded random word
NAMED_LIMBS = {
    SATURATING: [-128] * 8,
    0x7F7F7F7F7F7F7F7F: [127] * 8,
    0x8080808080808080: [-128] + [-127] * 7,
    0: [0] * 8,
    M64: [-1] + [0] * 7,
    1 << 63: [0] * 7 + [-128],
    0x80: [-128, 1] + [0] * 6,
}


def saturating_key(rows: int, cols: int) -> np.ndarray:
    return np.full((rows, cols), SATURATING, dtype=U)


def mixed_key(rows: int, cols: int, seed: int) -> np.ndarray:
    """word (r, t) is MIXED[(r + 3 t) mod 8], the eighth a random word of the seed"""
    which = ((np.arange(rows, dtype=np.int64)[:, None] + 3 * np.arange(cols, dtype=np.int64)[None, :]) & 7).astype(np.uint8)
    out = np.random.default_rng(seed).integers(0, 2 ** 64, (rows, cols), dtype=U)
    for i, x in enumerate(MIXED):
        out[which == i] = U(x)
    return out


def crafted_key(kind: str, rows: int, cols: int, seed: int = 0x6ED6E) -> np.ndarray:
    return saturating_key(rows, cols) if kind == "saturating" else mixed_key(rows, cols, seed)


def packing_blob(header, rows: np.ndarray) -> np.ndarray:
    """the wire blob load_packing_key takes: a real export's 48-byte header, then the rows"""
    head = np.frombuffer(bytes(header), dtype=np.uint8)
    assert len(head) == 48
    return np.concatenate([head, np.ascontiguousarray(rows, dtype="<u8").reshape(-1).view(np.uint8)])
