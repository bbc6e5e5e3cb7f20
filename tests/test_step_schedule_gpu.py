"""The blind rotation's packed step schedule (step_sched.h; fbr_rotate of fft_br.hip): the
latency, key-products and pair shapes build one entry per unskipped step in their prologue and
walk the table one entry ahead.  The edges of a walked table, at k = 1, N = 2048 (and the k = 2
latency shape, whose next-step table moved into the same region): an empty table, a table of one entry at either end,
idle runs at the start, across the 64-step words of the live masks and at the end, a whole idle
word, steps idle for one bootstrap of a pair only, an odd gate count.  Every output word is
compared with the oracle's.

The mask words are written directly: v 2^(64 - log2 2N) mod-switches to exactly v, 0 gives an
idle element.  Both compiled points (k = 1, N = 2048 and k = 2, N = 1024) share the fixture's
LWE dimension n = 742, which is even: the last pair is (a[740], a[741]) and the zero pad abar[n]
belongs to no step, so no supported point reaches the padded element of an odd n on the device.
"last_odd" leaves only a[741], the last pair's second element, non-zero; the build of an odd n's
last entry from the pad is covered on the host (tools/step_sched_check.cpp: n = 1, 63, 127, 129,
741, 1023, through the helpers the kernel calls)."""
import numpy as np
import pytest

import test_gate_programs as tg  # its oracles and device contexts, one per (point, environment)

pytestmark = pytest.mark.gpu

K1, K2 = "k1n2048", "k2n1024"
LATENCY, KP, PAIR = {"FR_FFT_KPRE_BATCH": 0}, {"FR_FFT_KPRE_BATCH": 64}, {"FR_FFT_SMALL_BATCH": 0}
NAMES = ["empty", "first", "first_even", "last", "last_odd", "runs", "alternate", "dense", "extremes"]
_ROWS = {}


def rows(request, pid):
    """(keyswitched rows by name, their LUTs, the oracle's output rows), once per point"""
    if pid not in _ROWS:
        O = tg.oracle(request, pid)
        n, steps = O.n, (O.n + 1) // 2
        shift = 64 - (int(O.P.N).bit_length())  # log2(2N) = bit_length(N)
        vmax = 2 * O.P.N - 1
        rng = np.random.default_rng(1234)
        dense = rng.integers(1, vmax, n, endpoint=True).astype(np.uint64) << np.uint64(shift)
        body = rng.integers(1, 2**64 - 1, len(NAMES), dtype=np.uint64)  # b-bar != 0 (the top bits are random)
        ks = {name: np.zeros(n + 1, dtype=np.uint64) for name in NAMES}
        ks["first"][0:2] = dense[0:2]
        ks["first_even"][0] = dense[0]
        ks["last"][n - 2:n] = dense[n - 2:n]
        ks["last_odd"][n - 1] = dense[n - 1]
        ks["runs"][:n] = dense
        # idle steps: the first five, a run across the word boundary at 64, the whole word
        # 192..255, a run in the middle, single ones at word edges, the last three
        for lo, hi in ((0, 5), (60, 70), (127, 128), (128, 129), (150, 170), (192, 256), (319, 321), (steps - 3, steps)):
            ks["runs"][2 * lo:2 * hi] = 0
        ks["alternate"][:n] = dense
        for t in range(0, steps, 2):
            ks["alternate"][2 * t:2 * t + 2] = 0
        ks["dense"][:n] = dense
        # the field edges: e = 1 and e = 2N - 1 at steps 0 and steps - 1, nothing between
        ks["extremes"][0], ks["extremes"][1] = np.uint64(vmax << shift), np.uint64(1 << shift)
        ks["extremes"][n - 2], ks["extremes"][n - 1] = np.uint64(1 << shift), np.uint64(vmax << shift)
        for i, name in enumerate(NAMES):
            ks[name][n] = body[i]
        luts = {name: [(5 * m + 3 * i + 1) % 16 for m in range(16)] for i, name in enumerate(NAMES)}
        want = {name: O.blind_rotate(ks[name], luts[name]) for name in NAMES}
        _ROWS[pid] = ks, luts, want
    return _ROWS[pid]


def check(ctx, data, names):
    """one launch of the named rows in this order: the names whose words differ from the oracle's"""
    ks, luts, want = data
    got = ctx.dev_blind_rotate(np.stack([ks[x] for x in names]), [luts[x] for x in names])
    return [(i, x) for i, x in enumerate(names) if not (got[i] == want[x]).all()]


@pytest.mark.parametrize("name", NAMES)
def test_latency_shape_single(request, key_blob, monkeypatch, name):
    """the latency shape, a lone bootstrap per edge"""
    ctx = tg.device_ctx(key_blob, monkeypatch, K1, LATENCY)
    assert not check(ctx, rows(request, K1), [name])


def test_latency_shape_batch(request, key_blob, monkeypatch):
    """every edge in one latency-shape launch: each workgroup builds and walks its own table"""
    ctx = tg.device_ctx(key_blob, monkeypatch, K1, LATENCY)
    assert not check(ctx, rows(request, K1), NAMES)


@pytest.mark.parametrize("names", [["empty"], ["runs"], ["last_odd"], ["extremes"], ["runs", "empty", "alternate"],
                                   ["first", "last", "dense"]], ids="+".join)
def test_key_products_shape(request, key_blob, monkeypatch, names):
    """the key-products shape at 1 and 3 gates: the producer stores nothing for an idle pair
    and the rotation's table never addresses one"""
    ctx = tg.device_ctx(key_blob, monkeypatch, K1, KP)
    assert not check(ctx, rows(request, K1), names)


@pytest.mark.parametrize("names", [["empty", "empty"], ["empty", "first"], ["last_odd", "empty"], ["runs", "dense"],
                                   ["alternate", "runs"], ["runs", "alternate", "last"], ["dense", "extremes", "empty"],
                                   ["first_even"]], ids="+".join)
def test_pair_shape(request, key_blob, monkeypatch, names):
    """the pair shape at 2 gates, and at 3 and 1 (an odd count: the last workgroup repeats its
    gate): a step runs when either bootstrap's pair is non-zero, with the other's exact zeros;
    an empty table when both masks are zero"""
    ctx = tg.device_ctx(key_blob, monkeypatch, K1, PAIR)
    assert not check(ctx, rows(request, K1), names)


@pytest.mark.parametrize("env", [LATENCY, KP, PAIR], ids=["latency", "kp", "pair"])
def test_multi_value_outputs(request, key_blob, monkeypatch, env):
    """a multi-value job (three LUTs of one rotation) on the row with idle runs: the pair shape
    stages abar in the rows that hold the multi-value terms after the loop"""
    O = tg.oracle(request, K1)
    ks, _, _ = rows(request, K1)
    luts = [[(3 * m + i) % 16 for m in range(16)] for i in range(3)]
    want = O.blind_rotate_multi(ks["runs"], luts)
    got = tg.device_ctx(key_blob, monkeypatch, K1, env).dev_blind_rotate_multi(ks["runs"], luts)
    assert (got == want).all()


def test_k2_latency_shape(request, key_blob, monkeypatch):
    """k = 2, N = 1024: its latency shape keeps the table of next unskipped steps, now inside the
    schedule's LDS region: the same edges"""
    ctx = tg.device_ctx(key_blob, monkeypatch, K2, {})
    assert not check(ctx, rows(request, K2), NAMES)
