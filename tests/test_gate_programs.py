"""Directed gate programs and blind-rotation edge rows, word for word against the oracle
in every compiled launch shape and in the keyswitch fallbacks.

tests/gate_programs.py builds two seeded gate programs (small: every level in the latency
shape; large: an odd level-1 job count above 256) whose gate mix is asserted below, and
the mask / body edge rows of the blind rotation's step-skip logic.  CPU: the generator
covers what it claims, the oracle alone decodes every gate to the generator's plaintext
value at both FFT points, and a wrong job kind changes the words but not the decryption.
GPU: fr_run_gates against Oracle.gates on every word of every gate, the launch shape of
each level read back from the device timers; dev_blind_rotate against Oracle.blind_rotate
on the edge rows.

Oracle time per (point, program), 8 threads: k1n2048 small 0.4 s, large 2.2 s; k2n1024
small 0.3 s, large 1.8 s; RNS small 12.2 s, so the RNS run is cut to level 1 of the small
program (44 of its 45 jobs).  Edge rows: 0.15 s per FFT point, 4.7 s on the RNS ring."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fheregex as F
import gate_programs as gp
import oracle_ffi as of

SEED = 42
POINTS = {"k1n2048": (1, 2048, F.RING_FFT), "k2n1024": (2, 1024, F.RING_FFT), "rns": (1, 2048, F.RING_RNS)}

_ORACLE, _PROGRAM, _EXPECTED, _EDGE, _CTX = {}, {}, {}, {}, {}


def oracle(request, pid):
    if pid not in _ORACLE:
        if pid == "k2n1024":
            _ORACLE[pid] = of.Oracle(request.getfixturevalue("fixture_key"), seed=SEED, k=2, N=1024, ring=of.RING_FFT)
        else:
            _ORACLE[pid] = request.getfixturevalue({"k1n2048": "oracle_k1", "rns": "oracle_rns"}[pid])
    return _ORACLE[pid]


def program(name):
    if name not in _PROGRAM:
        _PROGRAM[name] = gp.build(name[:5]).level1() if name.endswith("-level1") else gp.build(name)
    return _PROGRAM[name]


def expected(request, pid, name):
    """(input rows, every gate's expected row), once per (point, program)"""
    if (pid, name) not in _EXPECTED:
        O, p = oracle(request, pid), program(name)
        rows = p.content_rows(O)
        t = time.perf_counter()
        words = p.oracle_eval(O, rows)
        print("oracle %s %s: %.2f s" % (pid, name, time.perf_counter() - t))
        _EXPECTED[pid, name] = rows, words
    return _EXPECTED[pid, name]


def edge(request, pid):
    """(names, keyswitched rows, LUTs, expected rows) of the unique edge rows, once per point"""
    if pid not in _EDGE:
        O = oracle(request, pid)
        names, ks, luts = gp.edge_rows(O.n, O.P.N)
        t = time.perf_counter()
        with ThreadPoolExecutor(max(1, min(16, of.Oracle.num_threads()))) as ex:
            words = np.stack(list(ex.map(lambda i: O.blind_rotate(ks[i], luts[i]), range(len(names)))))
        print("oracle %s edge rows: %.2f s" % (pid, time.perf_counter() - t))
        _EDGE[pid] = names, ks, luts, words
    return _EDGE[pid]


# ------------------------------------------------------------------- CPU
def test_lut_catalogue():
    N, half = 2048, 2048 // 32
    assert of.lut_terms(N, gp.CONST0) == []
    assert of.lut_terms(N, gp.CONST1) == [(N - half, -2)]
    t = of.lut_terms(N, gp.ONES8)
    assert len(t) == 8 and {abs(d) for _, d in t} == {1} and gp.norm2(gp.ONES8) == 8
    assert sorted(d for _, d in of.lut_terms(N, gp.TWOS)) == [-2, 2] and gp.norm2(gp.TWOS) == 8
    assert gp.norm2(gp.NORM10) == 10
    assert all(gp.norm2(l) <= 8 for l in gp.SMALL_POOL)
    assert len({tuple(l) for l in gp.SMALL_POOL}) == len(gp.SMALL_POOL)
    # norm^2 is even for every LUT, so 10 is the least norm above the executor's bound of 8
    rng = np.random.default_rng(1)
    assert all(gp.norm2(list(rng.integers(0, 16, 16))) % 2 == 0 for _ in range(2000))


@pytest.mark.parametrize("name", ["small", "large"])
def test_programs_cover_the_gate_mix(name):
    p = program(name)
    assert p == gp.build(name), "the generator is a function of its seed"
    p.check_plain()
    G = p.gates
    jobs = p.jobs()
    assert len(jobs) == 2 and {g.level for g in G} == {1, 2}
    l1, l2 = jobs
    nin = lambda g: len(p.signature(g)[0])  # the device's n_in: trivial inputs are folded away
    g1 = [g for g in G if g.level == 1]
    lut1 = [g for g in g1 if g.kind == gp.LUT]
    sign = [g for g in g1 if g.kind == gp.SIGN]
    # n_in
    assert any(nin(g) == 0 and not g.ins for g in lut1) and any(nin(g) == 0 and not g.ins for g in sign)
    assert {nin(g) for g in lut1} >= set(range(17))
    assert any(len(g.ins) == 4 and {s[1] for s, _ in g.ins} == {g.ins[0][0][1]} and {s[2] for s, _ in g.ins} == {0, 1, 2, 3}
               for g in lut1)
    assert any(len(g.ins) == 2 and g.ins[0][0] == g.ins[1][0] and g.ins[0][1] != g.ins[1][1] for g in lut1)
    assert any(nin(g) == 16 and len({s[2] for s, _ in g.ins if s[1] == g.ins[0][0][1]}) == 4 for g in lut1)
    # weights and offsets
    assert {w for g in g1 for _, w in g.ins} >= {-128, 127, 0}
    assert {np.sign(g.offset) for g in lut1} == {-1, 0, 1} and {np.sign(g.offset) for g in sign} == {-1, 1}
    assert all(g.s == int(g.s) and 0 <= g.s < 16 for g in G if g.kind == gp.LUT)
    assert {g.s for g in lut1} >= {0, 15}
    assert {g.s for g in sign} >= {0.5, -0.5, 15.5, -15.5} and all(g.s % 1 == 0.5 and -16 < g.s < 16 for g in sign)
    g2 = [g for g in G if g.level == 2]
    assert {w for g in g2 for _, w in g.ins} <= {1, -1, 2, -2}
    assert all(any(s[0] == "g" for s, _ in g.ins) for g in g2) and any(s[0] == "c" for g in g2 for s, _ in g.ins)
    assert all(G[s[1]].level == 1 for g in g2 for s, _ in g.ins if s[0] == "g")
    # multi-value groups
    shape = lambda tag: [(j.kind, len(j.gates)) for j in l1 if G[j.gates[0]].tag == tag]
    reps = 1 if name == "small" else gp.LARGE_REPEATS
    for g in range(2, 8):
        assert shape("group%d" % g) == [(gp.MULTI, g)] * reps
    assert shape("group9") == [(gp.MULTI, 8), (gp.DIRECT, 1)] * reps
    assert shape("group10") == [(gp.MULTI, 8), (gp.MULTI, 2)] * reps
    assert shape("group17") == [(gp.MULTI, 8), (gp.MULTI, 8), (gp.DIRECT, 1)] * reps
    inter = [j for j in l1 if G[j.gates[0]].tag == "group3-interleaved"]
    assert len(inter) == reps and all(len(j.gates) == 3 and j.gates[2] - j.gates[0] > 2 for j in inter)
    mid = [j for j in l1 if G[j.gates[0]].tag == "group-norm10-middle"]
    assert [(j.kind, len(j.gates)) for j in mid] == [(gp.MULTI, 2), (gp.DIRECT, 1)] * reps
    assert all(a.gates[1] == a.gates[0] + 2 and b.gates == [a.gates[0] + 1] and gp.norm2(G[b.gates[0]].lut) == 10
               for a, b in zip(mid[0::2], mid[1::2]))
    in_multi = {tuple(G[gi].lut) for j in l1 if j.kind == gp.MULTI for gi in j.gates}
    assert in_multi >= {tuple(l) for l in gp.SPECIAL}
    assert all(gp.norm2(G[gi].lut) <= 8 for j in l1 + l2 if j.kind == gp.MULTI for gi in j.gates)
    assert all(len({tuple(G[gi].lut) for gi in j.gates}) == len(j.gates) for j in l1 + l2)
    # direct jobs: full-range LUTs, except the overflow gate of a group of 9 or 17
    direct = [G[j.gates[0]] for j in l1 if j.kind == gp.DIRECT]
    assert all(gp.norm2(g.lut) > 8 for g in direct if g.tag not in ("group9", "group17"))
    assert all(len({p.signature(G[gi]) for gi in j.gates}) == 1 for j in l1 + l2)
    # sign gates
    for fan in (1, 2, 15, 16):
        assert {g.value for g in sign if nin(g) == fan} == {0, 1}, fan
    # the trivial radix reaches every job kind
    for kind in (gp.MULTI, gp.DIRECT, gp.JSIGN):
        assert any(p.is_triv(s) for j in l1 if j.kind == kind for s, _ in G[j.gates[0]].ins), kind
    assert any(p.is_triv(s) for g in g2 for s, _ in g.ins)
    # job order: what meets in a pair workgroup
    kinds = [(j.kind, len(j.gates)) for j in l1]
    pairs = set(zip(kinds[0::2], kinds[1::2]))
    assert ((gp.MULTI, 8), (gp.JSIGN, 1)) in pairs and ((gp.JSIGN, 1), (gp.DIRECT, 1)) in pairs
    assert ((gp.DIRECT, 1), (gp.MULTI, 2)) in pairs
    assert any(a[0] == b[0] == gp.MULTI and a[1] != b[1] for a, b in pairs)
    # sizes
    if name == "small":
        assert len(l1) <= 64 and len(l2) == 1 and l2[0].kind == gp.MULTI
    else:
        assert len(l1) % 2 == 1 and 257 <= len(l1) <= 330 and kinds[-1] == (gp.MULTI, 8)
        assert {j.kind for j in l2} == {gp.MULTI, gp.DIRECT, gp.JSIGN} and len(l2) <= 256
    # the oracle's jobs keep the trivial inputs as rows; nothing exceeds its 16 inputs
    assert all(len(G[j.gates[0]].ins) <= 16 for j in l1 + l2)
    cut = p.level1()
    assert cut.gates == g1 and len(cut.jobs()) == 1


@pytest.mark.parametrize("N", [2048, 1024])
def test_edge_rows_are_what_they_claim(N):
    n = 742
    names, ks, luts = gp.edge_rows(n, N)
    assert 24 <= len(names) <= 32 and len(set(names)) == len(names) and ks.shape == (len(names), n + 1)
    L = (2 * N).bit_length() - 1
    sw = lambda x: of.lib().or_mod_switch(int(x), L)
    a = {nm: np.array([sw(x) for x in r]) for nm, r in zip(names, ks)}
    idle = {nm: (a[nm][:n].reshape(-1, 2) == 0).all(axis=1) for nm in names}
    assert idle["zero"].all() and idle["wrap"].all() and idle["wrap-mixed"].all()
    assert (ks[names.index("wrap")][:n] == np.uint64(2**64 - 1)).all()
    assert len(set(ks[names.index("wrap-mixed")][:n].tolist())) == 3
    for nm, busy in (("pair0", [0]), ("pair370", [370]), ("coef0", [0]), ("coef741", [370])):
        assert np.nonzero(~idle[nm])[0].tolist() == busy, nm
    assert np.count_nonzero(a["coef0"][:n]) == 1 and a["coef0"][0] and np.count_nonzero(a["coef741"][:n]) == 1 and a["coef741"][n - 1]
    assert idle["even-idle"][0::2].all() and not idle["even-idle"][1::2].any()
    assert idle["odd-idle"][1::2].all() and not idle["odd-idle"][0::2].any()
    gaps = np.diff(np.nonzero(~idle["idle-runs"])[0])
    assert (np.diff(gaps) == 1).all() and gaps[0] == 2 and len(gaps) > 20
    assert (a["all-N"][:n] == N).all()
    p0, pN = a["sum-0"][:n].reshape(-1, 2), a["sum-N"][:n].reshape(-1, 2)
    assert (p0.sum(axis=1) == 2 * N).all() and (pN.sum(axis=1) % (2 * N) == N).all() and (p0 > 0).all()
    v0 = a["alt-v0"][:n].reshape(-1, 2)
    assert ((v0 == 0).sum(axis=1) == 1).all() and (v0[0::2, 0] == 0).all() and (v0[1::2, 1] == 0).all()
    assert (a["alt-1-top"][0:n:2] == 1).all() and (a["alt-1-top"][1:n:2] == 2 * N - 1).all()
    assert (ks[names.index("alt-1-top")][1:n:2] == np.uint64(2**64 - 2**(63 - L) - 1)).all()
    tie = ks[names.index("ties")][:n]
    base = (tie >> np.uint64(64 - L)).astype(np.int64)
    assert (a["ties"][0:n:3] == base[0::3] + 1).all() and (a["ties"][1:n:3] == base[1::3]).all()
    assert (a["ties"][2:n:3] == base[2::3] + 1).all()
    assert (tie[0::3] & np.uint64(2**(64 - L) - 1) == np.uint64(2**(63 - L))).all()
    for b in (0, 1, N // 32 - 1, N // 32, N - 1, N, N + N // 32, 2 * N - 1):
        assert a["body-%d" % b][n] == b
    assert a["body-wrap"][n] == 0 and ks[names.index("body-wrap")][n] == np.uint64(2**64 - 1)
    assert not idle["random0"].any() and not idle["random1"].any()
    order = gp.edge_order(names, 259)
    assert len(order) == 259 and set(order) == set(range(len(names))) and names[order[-1]] == "zero"
    assert [(names[x], names[y]) for x, y in zip(order[0:12:2], order[1:12:2])] == gp.EDGE_HEAD


@pytest.mark.parametrize("pid", ["k1n2048", "k2n1024"])
@pytest.mark.parametrize("name", ["small", "large"])
def test_oracle_decodes_every_gate(request, pid, name):
    """The reference alone is right on these inputs: every gate of the program decodes to
    the generator's plaintext value."""
    O, p = oracle(request, pid), program(name)
    _, words = expected(request, pid, name)
    got = O.decode16(words)
    bad = [(i, g.tag, int(got[i]), g.value) for i, g in enumerate(p.gates) if got[i] != g.value]
    assert len(got) == len(p.gates) and not bad, bad[:10]


def test_job_kind_changes_words_not_decryption(request):
    """Negative control: a group evaluated as separate direct jobs decodes to the same
    values, but its words differ from the multi-value evaluation's (all but the constant-0
    LUT's, whose output is the zero row either way).  A decrypt-only test cannot see a
    wrong job kind; the word comparison can."""
    O, p = oracle(request, "k1n2048"), program("small")
    rows, words = expected(request, "k1n2048", "small")
    job = p.jobs()[0][0]
    assert job.kind == gp.MULTI and len(job.gates) == 8 and p.gates[job.gates[0]].tag == "group8-special"
    slots = np.concatenate([rows, words])
    sep = O.gates([p.oracle_job(job, kind=gp.DIRECT, gates=[gi]) for gi in job.gates], slots)
    assert [int(x) for x in O.decode16(sep)] == [p.gates[gi].value for gi in job.gates]
    for q, gi in enumerate(job.gates):
        same = bool((sep[q] == words[gi]).all())
        assert same == (p.gates[gi].lut == gp.CONST0), (q, gi)
    assert not words[job.gates[0]].any()


# ------------------------------------------------------------------- GPU
def device_ctx(key_blob, monkeypatch, pid, env):
    """A context whose launch-shape limits come from FR_* (read at creation); one per
    (point, environment) for both GPU tables."""
    key = (pid, tuple(sorted(env.items())))
    if key not in _CTX:
        k, N, ring = POINTS[pid]
        for name, v in env.items():
            monkeypatch.setenv(name, str(v))
        ctx = F.Context(device=0, params=F.default_params(k=k, N=N, ring=ring))
        for name in env:
            monkeypatch.delenv(name)
        ctx.load_client_key(key_blob)
        ctx.gen_server_key(SEED)
        _CTX[key] = ctx
    return _CTX[key]


LAT, PAIR, WIDE = "latency", "pair", "one bootstrap per workgroup"  # what the device timers tell apart

# environment, point, program, shape of each level, E of the throughput geometry (FFT ring)
PROGRAM_ROWS = [
    ({}, "k1n2048", "small", (LAT, LAT), 4),
    ({}, "k2n1024", "small", (LAT, LAT), 8),
    ({}, "rns", "small-level1", (LAT,), None),                        # its small-batch kernel
    ({}, "k1n2048", "large", (PAIR, LAT), 4),                          # pair, lone tail
    ({}, "k2n1024", "large", (WIDE, LAT), 8),                          # throughput E = 8
    ({"FR_FFT_PAIR_BATCH": 0}, "k1n2048", "large", (WIDE, LAT), 4),    # throughput E = 4
    ({"FR_FFT_DUAL": 1}, "k1n2048", "large", (WIDE, LAT), 4),          # dual
    ({"FR_FFT_LANE_ELEMS": 4}, "k2n1024", "large", (WIDE, LAT), 4),    # throughput k = 2, E = 4
    ({"FR_FFT_SMALL_BATCH": 0}, "k1n2048", "small", (PAIR, PAIR), 4),  # the one-job level: a lone pair workgroup
    ({"FR_FFT_SMALL_BATCH": 0}, "k2n1024", "small", (WIDE, WIDE), 8),
    ({"FR_KS_MFMA": 0}, "k1n2048", "small", (LAT, LAT), 4),            # VALU keyswitch, 64 K slices
    ({"FR_KS_MFMA": 0}, "k1n2048", "large", (PAIR, LAT), 4),           # VALU keyswitch, 16 K slices
    ({"FR_KS_LDS": 0}, "k1n2048", "large", (PAIR, LAT), 4),            # k_ks_mfma<4, 1>
]
row_id = lambda r: "-".join(["%s=%s" % kv for kv in r[0].items()] or ["default"]) + "-%s-%s" % (r[1], r[2])


@pytest.mark.gpu
@pytest.mark.parametrize("row", PROGRAM_ROWS, ids=row_id)
def test_gate_program_words(request, key_blob, monkeypatch, row):
    """fr_run_gates on the program: block 0 of every gate equals the oracle's row word for
    word, and each level ran in the shape the table names (device timer deltas)."""
    env, pid, name, shapes, E = row
    p = program(name)
    rows, words = expected(request, pid, name)
    ctx = device_ctx(key_blob, monkeypatch, pid, env)
    if E is not None:
        assert "ring=fft E=%d " % E in ctx.info()
    hs = p.upload(ctx, rows)
    ctx.set_profiling(1)
    t0 = ctx.device_timers()
    outs = ctx.run_gates(p.fr_gates(hs))
    t1 = ctx.device_timers()
    ctx.set_profiling(0)
    got = np.stack([ctx.download_radix(h)[0] for h in outs])
    for h in outs + hs:
        ctx.release(h)
    jobs = p.jobs()
    job_of = {gi: (l + 1, q, j.kind, len(j.gates)) for l, jl in enumerate(jobs) for q, j in enumerate(jl) for gi in j.gates}
    bad = [(gi, p.gates[gi].tag) + job_of[gi] for gi in range(len(p.gates)) if not (got[gi] == words[gi]).all()]
    assert not bad, (len(bad), bad[:12])
    d = {k: t1[k] - t0[k] for k in ("br_launches", "br_gates", "lat_gates", "pair_gates")}
    sizes = [len(jl) for jl in jobs]
    assert len(shapes) == len(sizes)
    assert d == {"br_launches": len(sizes), "br_gates": sum(sizes),
                 "lat_gates": sum(n for n, s in zip(sizes, shapes) if s == LAT),
                 "pair_gates": sum(n for n, s in zip(sizes, shapes) if s == PAIR)}, (d, sizes)


EDGE_ROWS = [
    ({}, "k1n2048", 0),                          # latency: the unique rows once
    ({}, "k2n1024", 0),
    ({}, "rns", 0),
    ({}, "k1n2048", 259),                        # pair
    ({}, "k2n1024", 259),                        # throughput E = 8
    ({"FR_FFT_PAIR_BATCH": 0}, "k1n2048", 259),  # throughput E = 4
    ({"FR_FFT_DUAL": 1}, "k1n2048", 259),        # dual
    ({"FR_FFT_LANE_ELEMS": 4}, "k2n1024", 259),  # throughput k = 2, E = 4
    ({"FR_FFT_SMALL_BATCH": 0}, "k1n2048", 41),  # pair on a small launch
    ({"FR_FFT_SMALL_BATCH": 0}, "k2n1024", 41),  # throughput on a small launch
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", EDGE_ROWS, ids=lambda r: row_id(r[:2] + (r[2] or "unique",)))
def test_edge_rows_words(request, key_blob, monkeypatch, row):
    """dev_blind_rotate (direct LUTs) on the mask and body edge rows against
    Oracle.blind_rotate: idle ladders, idle pairs, exponents that cancel, rounding ties and
    bodies on LUT box boundaries.  A large launch repeats the unique rows (same row, same
    LUT) behind the workgroup pairs of gate_programs.EDGE_HEAD and ends on the all-zero
    row alone."""
    env, pid, count = row
    names, ks, luts, words = edge(request, pid)
    order = gp.edge_order(names, count) if count else list(range(len(names)))
    ctx = device_ctx(key_blob, monkeypatch, pid, env)
    got = ctx.dev_blind_rotate(ks[order], luts[order])
    bad = [(i, names[u]) for i, u in enumerate(order) if not (got[i] == words[u]).all()]
    assert not bad, (len(bad), bad[:12])
