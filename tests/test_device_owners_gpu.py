"""The Device class's resource owners on the GPU (both FFT points): a lane's keyswitch scratch,
digit rows and content-map ring outgrowing their first sizes, the lane set shrinking and
growing between matches, and a context torn down with lanes, cached plans, unresolved timers
and queued matches all live.

Every comparison is word for word against one-lane matches of the same ciphertexts under the
same seeded server key, computed once per point; the first of them is itself checked against
the oracle's evaluation of the match's schedule.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import fheregex as F
import oracle_ffi as of

pytestmark = pytest.mark.gpu

SEED = 42
PATTERN = "/abc/"
CHARS = 64
BATCH = 17
POINTS = [(F.RING_FFT, 1, 2048), (F.RING_FFT, 2, 1024)]
POINT_IDS = ["fft", "fft-k2n1024"]


def make(point, key_blob, device=0):
    ring, k, N = point
    ctx = F.Context(device=device, params=F.default_params(k=k, N=N, ring=ring))
    ctx.load_client_key(key_blob)
    if device >= 0:
        ctx.gen_server_key(SEED)
    return ctx


def words(ctx, hs):
    out, _ = ctx.has_match(hs, PATTERN)
    w = ctx.download_radix(out)
    ctx.release(out)
    return w


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def ref(request, key_blob, fixture_key):
    """BATCH distinct CHARS-character contents (every third holds the pattern), their
    ciphertexts, and each one's has_match words at one lane."""
    point = request.param
    rng = np.random.default_rng(97)
    texts = []
    for i in range(BATCH):
        t = "".join(chr(c) for c in rng.integers(0x20, 0x7F, CHARS)).replace("a", "x")
        texts.append(t[:3 * i + 2] + "abc" + t[3 * i + 5:] if i % 3 == 0 else t)
    assert len(set(texts)) == BATCH and all(len(t) == CHARS for t in texts)
    ctx = make(point, key_blob)
    cts = [ctx.encrypt_str(t, seed=300 + i) for i, t in enumerate(texts)]
    want = []
    for ct in cts:
        hs = ctx.upload_radix(ct)
        want.append(words(ctx, hs))
        for h in hs:
            ctx.release(h)
    assert [ctx.decrypt_radix(w) for w in want] == [int(i % 3 == 0) for i in range(BATCH)]
    ctx.close()
    ring, k, N = point
    O = of.Oracle(fixture_key, seed=SEED, k=k, N=N, ring=ring)
    S = F.schedule_match(CHARS, PATTERN)
    assert np.array_equal(want[0][0], O.run_schedule(S, cts[0])) and not want[0][1:].any()
    return SimpleNamespace(point=point, cts=cts, want=want, schedule=S)


def test_lane_scratch_and_content_map_grow(ref, key_blob):
    """One batch of 17 matches on a lane is wider than the lane's first keyswitch scratch (1,024
    gates), digit rows (1,024) and content map (4,096 entries), so all three are reallocated on
    the lane; then a single match binds a smaller map on the grown ring, and the context goes
    back to one lane."""
    widest = int(np.diff(ref.schedule.level_off).max())
    assert BATCH * widest > 1024 and 4 * CHARS * BATCH > 4096
    ctx = make(ref.point, key_blob)
    hss = [ctx.upload_radix(ct) for ct in ref.cts]
    ctx.set_lanes(2)
    for lane in (1, 2):  # consecutive asynchronous matches take consecutive lanes: both grow
        outs, st = ctx.has_match_batch(hss, PATTERN)
        assert st.blind_rotations == BATCH * len(ref.schedule.jobs) and st.plan_cached == 0
        for i, o in enumerate(outs):
            assert np.array_equal(ctx.download_radix(o), ref.want[i]), (lane, i)
            ctx.release(o)
    assert np.array_equal(words(ctx, hss[3]), ref.want[3])
    ctx.set_lanes(1)
    assert np.array_equal(words(ctx, hss[6]), ref.want[6])
    ctx.close()


def test_lane_set_shrinks_and_grows(ref, key_blob):
    """Asynchronous matches before and after lanes are released and created again; the output
    handles and slots released by one group are reused by the next."""
    ctx = make(ref.point, key_blob)
    hss = [ctx.upload_radix(ct) for ct in ref.cts[:3]]
    for lanes, count in ((4, 6), (2, 4), (3, 4)):
        ctx.set_lanes(lanes)
        outs = [ctx.has_match(hss[i % 3], PATTERN)[0] for i in range(count)]
        for i, o in enumerate(outs):
            assert np.array_equal(ctx.download_radix(o), ref.want[i % 3]), (lanes, i)
            ctx.release(o)
    ctx.set_lanes(1)
    assert np.array_equal(words(ctx, hss[1]), ref.want[1])
    ctx.close()


def test_teardown_with_everything_live(ref, key_blob):
    """close() with three lanes set, a cached plan on each, a compact-content upload's staging
    ring, level-2 timers never resolved and matches enqueued but never downloaded; a fresh
    context on the device then computes the reference's words."""
    ctx = make(ref.point, key_blob)
    hss = [ctx.upload_radix(ct) for ct in ref.cts[:3]]
    ctx.set_lanes(3)
    for i in range(3):  # one plan per lane
        assert np.array_equal(words(ctx, hss[i]), ref.want[i])
    assert ctx.plan_cache_stats()["entries"] == 3
    client = make(ref.point, key_blob, device=-1)
    assert len(ctx.upload_compact_str(client.encrypt_str_compact("torn down", bytes(range(32))))) == 9
    ctx.set_profiling(2)
    for i in range(6):
        _, st = ctx.has_match(hss[i % 3], PATTERN)
        assert st.plan_cached == 1
    ctx.close()
    fresh = make(ref.point, key_blob)
    hs = fresh.upload_radix(ref.cts[0])
    assert np.array_equal(words(fresh, hs), ref.want[0])
    fresh.close()
