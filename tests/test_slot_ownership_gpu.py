"""Arena-slot accounting on the GPU (both FFT points): every operation that allocates slots gives
them back once its handles are released, and a call refused on the host leaves none behind.

`in_use` is Context.arena_stats()'s slots - free_slots after a synchronisation of every lane;
`held` is in_use minus the slots the plan cache accounts for.  Every operation's result is
decrypted and compared with its plaintext value first, so nothing passes by doing nothing.  No
case makes a launch or a HIP call fail: the refused calls are refused by host-side checks.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fheregex as F

pytestmark = pytest.mark.gpu

SEED = 42
PATTERN = "/abc/"
TEXT = "xyabcdzq"  # 8 characters, holds the pattern
OTHERS = ["abxcabxc", "zzzzzabc"]  # no match, match at the end
POINTS = [(F.RING_FFT, 1, 2048), (F.RING_FFT, 2, 1024)]
POINT_IDS = ["fft", "fft-k2n1024"]
KEY32 = bytes(range(32))


def make(point, key_blob):
    ring, k, N = point
    ctx = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
    ctx.load_client_key(key_blob)
    ctx.gen_server_key(SEED)
    ctx.set_plan_cache(0)  # the operations that cache a plan turn the cache on and off again
    return ctx


def in_use(ctx):
    s = ctx.arena_stats()
    return s["slots"] - s["free_slots"]


def held(ctx):
    return in_use(ctx) - ctx.plan_cache_stats()["slots"]


def dec(ctx, h):
    return ctx.decrypt_radix(ctx.download_radix(h))


def released(ctx):
    """a handle that was live and is not any more (valid until the next handle is made)"""
    h = ctx.trivial(0)
    ctx.release(h)
    return h


def new_env(point, key_blob):
    ctx = make(point, key_blob)
    hs = ctx.upload_radix(ctx.encrypt_str(TEXT, seed=1))
    bits = [0, 1, 0, 0]
    bools = ctx.upload_bool(ctx.encrypt_blocks(bits, seed=2))
    triv0 = ctx.or_many([])  # a trivial boolean 0
    e = SimpleNamespace(ctx=ctx, hs=hs, bits=bits, bools=bools, triv0=triv0, base=hs + bools + [triv0])
    e.want = match_words(e)
    return e


def match_words(e):
    out, _ = e.ctx.has_match(e.hs, PATTERN)
    w = e.ctx.download_radix(out)
    e.ctx.release(out)
    return w


@pytest.fixture(scope="module", params=POINTS, ids=POINT_IDS)
def env(request, key_blob):
    e = new_env(request.param, key_blob)
    assert e.ctx.decrypt_radix(e.want) == 1
    yield e
    e.ctx.close()


# ---- the table: each operation checks its result and returns the handles it made
def op_upload_radix(e):
    hs = e.ctx.upload_radix(e.ctx.encrypt_str("Hi!", seed=5))
    assert [dec(e.ctx, h) for h in hs] == [ord(c) for c in "Hi!"]
    return hs


def op_upload_bool(e):
    hs = e.ctx.upload_bool(e.ctx.encrypt_blocks([1, 0, 1], seed=6))
    assert [dec(e.ctx, h) for h in hs] == [1, 0, 1]
    return hs


def op_encrypt_upload_str(e):
    hs = e.ctx.encrypt_upload_str("dev", seed=7)
    assert [dec(e.ctx, h) for h in hs] == [ord(c) for c in "dev"]
    return hs


def op_upload_compact_str(e):
    hs = e.ctx.upload_compact_str(e.ctx.encrypt_str_compact("seed", KEY32))
    assert [dec(e.ctx, h) for h in hs] == [ord(c) for c in "seed"]
    return hs


def op_upload_compact_blocks(e):
    hs = e.ctx.upload_compact_blocks(e.ctx.encrypt_blocks_compact([1, 0, 0, 1, 1], KEY32))
    assert [dec(e.ctx, h) for h in hs] == [1, 0, 0, 1, 1]
    return hs


def op_trivial(e):
    h = e.ctx.trivial(0xA7)
    assert dec(e.ctx, h) == 0xA7
    return [h]


def cmp_const(name, c, want):
    def op(e):
        h = getattr(e.ctx, name)(e.hs[2], c)  # 'a' = 0x61
        assert dec(e.ctx, h) == want
        return [h]
    return op


def bool_op(name, i, j):
    def op(e):
        h = getattr(e.ctx, name)(e.bools[i], e.bools[j])
        assert dec(e.ctx, h) == (e.bits[i] & e.bits[j] if name == "and_" else e.bits[i] | e.bits[j])
        return [h]
    return op


def radix_op(name):
    def op(e):
        a, b = ord(TEXT[0]), ord(TEXT[3])
        h = getattr(e.ctx, name)(e.hs[0], e.hs[3])
        assert dec(e.ctx, h) == (a & b if name == "and_" else a | b)
        return [h]
    return op


def op_not_bool(e):
    h = e.ctx.not_(e.bools[0])
    assert dec(e.ctx, h) == 1 - e.bits[0]
    return [h]


def op_not_trivial_bool(e):
    h = e.ctx.not_(e.triv0)
    assert dec(e.ctx, h) == 1
    return [h]


def op_not_radix(e):
    h = e.ctx.not_(e.hs[1])
    assert dec(e.ctx, h) == ord(TEXT[1]) ^ 1
    return [h]


def or_many(n, with_one):
    """n inputs, the last a trivial 0 (n = 1: the lone encrypted input is copied)"""
    def op(e):
        vals = [int(with_one and i == (n - 1) // 2) for i in range(n - 1)] if n > 1 else [1]
        ins = e.ctx.upload_bool(e.ctx.encrypt_blocks(vals, seed=8 + n))
        h = e.ctx.or_many(ins + ([e.triv0] if n > 1 else []))
        assert dec(e.ctx, h) == int(any(vals))
        return ins + [h]
    return op


def op_or_many_trivial_only(e):
    h = e.ctx.or_many([e.triv0])
    assert dec(e.ctx, h) == 0
    return [h]


def op_or_each(e):
    hs = e.ctx.or_each([e.bools[:2], e.bools[2:], [e.bools[1]]])
    assert [dec(e.ctx, h) for h in hs] == [1, 0, 1]
    return hs


def op_run_gates(e):
    g0, g1 = F.Gate(), F.Gate()  # g0 = [low nibble of 'a' == 1], g1 = NOT g0
    g0.n_in, g0.kind = 2, F.GATE_LUT
    for q, (blk, w) in enumerate(((0, 1), (1, 4))):
        g0.in_[q], g0.in_block[q], g0.in_w[q] = e.hs[2], blk, w
    g0.lut[1] = 1
    g1.n_in, g1.kind = 1, F.GATE_LUT
    g1.in_[0], g1.in_w[0] = 0x80000000, 1
    g1.lut[0] = 1
    hs = e.ctx.run_gates([g0, g1])
    assert [dec(e.ctx, h) for h in hs] == [1, 0]
    return hs


def op_has_match_uncached(e):
    out, st = e.ctx.has_match(e.hs, PATTERN)
    assert dec(e.ctx, out) == 1 and st.plan_cached == 0 and e.ctx.plan_cache_stats()["entries"] == 0
    return [out]


def op_has_match_cached(e):
    ctx, before = e.ctx, held(e.ctx)
    ctx.set_plan_cache(8)
    for cached in (0, 1):
        out, st = ctx.has_match(e.hs, PATTERN)
        assert dec(ctx, out) == 1 and st.plan_cached == cached
        ctx.release(out)
        pc = ctx.plan_cache_stats()
        assert pc["entries"] == 1 and pc["slots"] == st.pbs > 0
        assert held(ctx) == before  # the cache accounts for every slot the plan keeps
    ctx.set_plan_cache(0)
    assert ctx.plan_cache_stats()["slots"] == 0
    return []


def op_has_match_parts(e):
    outs, _ = e.ctx.has_match_parts(np.array(e.hs, dtype=np.uint32), PATTERN, 0, len(TEXT), 4)
    assert 1 <= len(outs) <= 4 and max(dec(e.ctx, h) for h in outs) == 1
    return outs


def op_has_match_batch(e):
    extra = [e.ctx.upload_radix(e.ctx.encrypt_str(t, seed=20 + i)) for i, t in enumerate(OTHERS)]
    outs, _ = e.ctx.has_match_batch([e.hs] + extra, PATTERN)
    assert [dec(e.ctx, h) for h in outs] == [1, 0, 1]
    return outs + [h for hs in extra for h in hs]


def op_async_lanes(e):
    ctx, before = e.ctx, held(e.ctx)
    ctx.set_plan_cache(8)
    ctx.set_lanes(2)
    outs = [ctx.has_match(e.hs, PATTERN)[0] for _ in range(4)]  # two per lane: a miss and a hit each
    assert [dec(ctx, h) for h in outs] == [1] * 4
    for h in outs:
        ctx.release(h)
    assert ctx.plan_cache_stats()["entries"] == 2 and held(ctx) == before
    ctx.set_lanes(1)  # the lanes' plan copies go with the lanes
    assert ctx.plan_cache_stats()["entries"] == 0
    ctx.set_plan_cache(0)
    return []


def op_shard_plan(e):
    before = in_use(e.ctx)
    P = F.ShardPlan(e.ctx, e.hs, PATTERN)
    assert in_use(e.ctx) == before + P.stats.pbs
    for l in range(P.levels):
        P.run(l, 0, P.jobs(l))
    out, _ = P.finish()
    assert dec(e.ctx, out) == 1
    P.free()
    return [out]


def op_export_import_bool_device(e):
    ctx = e.ctx
    triv1 = ctx.not_(e.triv0)
    hs = [e.bools[1], triv1, e.triv0, e.bools[0]]
    buf = torch.zeros(len(hs) * ctx.lwe_len, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.export_bool_device(hs, buf.data_ptr())
    back = ctx.import_bool_device(buf.data_ptr(), len(hs))
    assert [dec(ctx, h) for h in back] == [e.bits[1], 1, 0, e.bits[0]]
    return back + [triv1]


IDENT = list(range(16))
LUTS = [[int(v == 6) for v in range(16)], [int(v in (6, 13)) for v in range(16)], [int(v >= 9) for v in range(16)]]


def op_dev_keyswitch_blind_rotate(e):
    ks = e.ctx.dev_keyswitch(e.ctx.encrypt_blocks([9, 4], seed=30))
    out = e.ctx.dev_blind_rotate(ks, [IDENT, [15 - v for v in IDENT]])
    assert [e.ctx.decode_block(o) for o in out] == [9, 11]
    return []


def op_dev_blind_rotate_multi(e):
    ks = e.ctx.dev_keyswitch(e.ctx.encrypt_blocks([13], seed=31))
    out = e.ctx.dev_blind_rotate_multi(ks[0], LUTS)
    assert [e.ctx.decode_block(o) for o in out] == [l[13] for l in LUTS]
    return []


def op_dev_bench_pbs(e):
    br, total = e.ctx.dev_bench_pbs([e.hs[0], e.hs[5], e.bools[1]], 1)
    assert 0 < br <= total
    return []


TABLE = {
    "upload_radix": op_upload_radix, "upload_bool": op_upload_bool, "encrypt_upload_str": op_encrypt_upload_str,
    "upload_compact_str": op_upload_compact_str, "upload_compact_blocks": op_upload_compact_blocks,
    "trivial": op_trivial,
    "eq_const": cmp_const("eq_const", 0x61, 1), "gt_const": cmp_const("gt_const", 0x61, 0),
    "le_const": cmp_const("le_const", 0x61, 1),
    "and_bool": bool_op("and_", 1, 0), "or_bool": bool_op("or_", 1, 0),
    "and_radix": radix_op("and_"), "or_radix": radix_op("or_"),
    "not_bool": op_not_bool, "not_trivial_bool": op_not_trivial_bool, "not_radix": op_not_radix,
    "or_many_1": or_many(1, True), "or_many_1_trivial": op_or_many_trivial_only, "or_many_2": or_many(2, True),
    "or_many_17": or_many(17, True), "or_many_40": or_many(40, True), "or_many_40_zero": or_many(40, False),
    "or_each": op_or_each, "run_gates": op_run_gates,
    "has_match_uncached": op_has_match_uncached, "has_match_cached": op_has_match_cached,
    "has_match_parts": op_has_match_parts, "has_match_batch": op_has_match_batch, "async_lanes": op_async_lanes,
    "shard_plan": op_shard_plan, "export_import_bool_device": op_export_import_bool_device,
    "dev_keyswitch_blind_rotate": op_dev_keyswitch_blind_rotate, "dev_blind_rotate_multi": op_dev_blind_rotate_multi,
    "dev_bench_pbs": op_dev_bench_pbs,
}


def run_op(e, name):
    before = held(e.ctx)
    for h in TABLE[name](e):
        e.ctx.release(h)
    assert held(e.ctx) == before, name


@pytest.mark.parametrize("name", list(TABLE))
def test_path_gives_its_slots_back(env, name):
    run_op(env, name)


def test_second_pass_takes_no_new_slots_and_nothing_stays(request, key_blob):
    """The whole table twice on a fresh context of each point: the second pass does not raise the
    arena's high-water mark, and with every handle released nothing is in use."""
    for point in POINTS:
        e = new_env(point, key_blob)
        for name in TABLE:
            run_op(e, name)
        slots = e.ctx.arena_stats()["slots"]
        for name in TABLE:
            run_op(e, name)
        assert e.ctx.arena_stats()["slots"] == slots
        for h in e.base:
            e.ctx.release(h)
        assert e.ctx.plan_cache_stats()["slots"] == 0 and in_use(e.ctx) == 0
        e.ctx.close()


# ---- calls refused on the host before any launch
def bad_bench_pbs(e):
    e.ctx.dev_bench_pbs([e.hs[0], e.hs[1], released(e.ctx)], 1)


def bad_match_bool_content(e):
    e.ctx.has_match(e.hs[:3] + [e.bools[0]] + e.hs[4:], PATTERN)


def bad_match_absent_position(e):
    e.ctx.has_match(e.hs[:3] + [F.NULL_CT] + e.hs[4:], PATTERN)


def bad_or_many(e):
    e.ctx.or_many([e.bools[0], e.hs[0]])


def bad_run_gates(e):
    g0, g1 = F.Gate(), F.Gate()
    g0.n_in, g0.kind = 1, F.GATE_LUT
    g0.in_[0], g0.in_w[0] = 0x80000001, 1  # reads gate 1
    g1.n_in, g1.kind = 1, F.GATE_LUT
    g1.in_[0], g1.in_block[0], g1.in_w[0] = e.hs[0], 0, 1
    e.ctx.run_gates([g0, g1])


def bad_export(e):
    buf = torch.zeros(3 * e.ctx.lwe_len, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    triv1 = e.ctx.not_(e.triv0)
    try:
        e.ctx.export_bool_device([e.triv0, triv1, released(e.ctx)], buf.data_ptr())
    finally:
        e.ctx.release(triv1)


def bad_and(e):
    e.ctx.and_(e.hs[0], released(e.ctx))


REFUSED = {"dev_bench_pbs": bad_bench_pbs, "has_match_bool_content": bad_match_bool_content,
           "has_match_absent_position": bad_match_absent_position, "or_many_bool_and_radix": bad_or_many,
           "run_gates_reads_later_gate": bad_run_gates, "export_bool_device_released": bad_export,
           "and_released": bad_and}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_call_leaves_nothing(env, name):
    before = in_use(env.ctx)
    with pytest.raises(F.FheRegexError) as ei:
        REFUSED[name](env)
    assert type(ei.value) is F.FheRegexError and ei.value.code == F.ERR_INVALID
    print(f"{name}: slots held after the refusal: {in_use(env.ctx) - before}")
    assert in_use(env.ctx) == before
    assert np.array_equal(match_words(env), env.want)
