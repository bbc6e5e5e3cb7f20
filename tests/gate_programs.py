"""Directed gate programs and blind-rotation edge rows for tests/test_gate_programs.py
(no GPU use, no test functions; tests/regex_fuzz.py is the precedent).

A seeded Program is plain data: input values and gates.  From that one description come
(a) the fheregex.Gate array for Context.run_gates, (b) the oracle's job list for
Oracle.gates, level by level, and (c) the plaintext value of every gate.  The job list
restates the executor's merge rule (plan.h build_schedule) in Program.jobs; a wrong
restatement shows as a failing word comparison, never as a silent pass.

The norm^2 of a LUT's multi-value factor w_f is always even: its coefficients sum to
(lut[15] - lut[0]) - (lut[0] + lut[15]) = -2 lut[0], and d^2 = d (mod 2).  So the
executor's boundary "norm^2 <= 8 joins" lies between 8 and 10; NORM10 is the smallest
LUT norm that must not join (no LUT has norm^2 = 9).
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

import fheregex as F
import oracle_ffi as of

LUT, SIGN = F.GATE_LUT, F.GATE_SIGN
MULTI, DIRECT, JSIGN = 0, 1, 2  # or_gate.direct / fr_job.kind
MV_MAX_NORM2 = 8
MAX_OUT = 8
GATE_REF = 0x80000000


def norm2(lut) -> int:
    """sum of the squared w_f coefficients (their positions depend on N, they do not)"""
    return sum(d * d for _, d in of.lut_terms(2048, lut))


CONST0 = [0] * 16                               # no terms
CONST1 = [1] * 16                               # one term, -2 at N - half
ONES8 = [0, 1, 0, 1, 0, 1, 0, 1] + [0] * 8      # 8 terms of +-1: norm^2 8
TWOS = [0, 0, 0, 2, 2, 2, 2] + [0] * 9          # steps +2, -2: norm^2 8
NORM10 = [0, 1, 0, 1, 0, 1, 0, 1, 0] + [1] * 7  # 9 steps of +-1 and the wrap term -1: norm^2 10
SPECIAL = [CONST0, CONST1, ONES8, TWOS]
# distinct LUTs of norm^2 <= 8 for the groups
SMALL_POOL = (SPECIAL + [[int(v == c) for v in range(16)] for c in range(16)]
              + [[int(v >= c) for v in range(16)] for c in range(1, 15)]
              + [[2 * int(v == c) for v in range(16)] for c in range(16)])


@dataclass
class Gate:
    ins: list          # [(src, w)]; src = ("c", input, block) or ("g", gate index)
    offset: int        # units of Delta/2
    kind: int          # LUT or SIGN
    lut: list
    level: int
    s: float           # plaintext offset/2 + sum w m: LUT in [0, 16), sign a half-integer in (-16, 16)
    value: int
    tag: str = ""      # what the gate is in the program for (the coverage test reads it)


@dataclass
class Job:
    gates: list        # gate indices, output order
    kind: int          # MULTI, DIRECT or JSIGN


@dataclass
class Program:
    name: str
    seed: int
    radix: list                       # byte values: fresh radix ciphertexts (four base-4 blocks)
    bools: list                       # bits: fresh booleans
    triv: int                         # byte value of the one trivial radix
    gates: list = field(default_factory=list)

    # -- inputs
    @property
    def triv_input(self):
        return len(self.radix) + len(self.bools)

    def is_triv(self, src):
        return src[0] == "c" and src[1] == self.triv_input

    def row(self, inp, blk):
        """content row of (input, block): radix blocks, booleans, the trivial radix's blocks"""
        R, B = len(self.radix), len(self.bools)
        if inp < R:
            return 4 * inp + blk
        if inp < R + B:
            assert blk == 0
            return 4 * R + (inp - R)
        return 4 * R + B + blk

    @property
    def n_rows(self):
        return 4 * len(self.radix) + len(self.bools) + 4

    def message(self, inp, blk):
        R, B = len(self.radix), len(self.bools)
        if inp < R:
            return (self.radix[inp] >> (2 * blk)) & 3
        if inp < R + B:
            return self.bools[inp - R]
        return (self.triv >> (2 * blk)) & 3

    def plain(self, src):
        return self.message(src[1], src[2]) if src[0] == "c" else self.gates[src[1]].value

    def content_rows(self, O) -> np.ndarray:
        """the inputs as LWE rows under the oracle's key: fresh encryptions, then the
        trivial radix as trivial rows (not folded: the host's off += 2 w triv is checked)"""
        R, B = len(self.radix), len(self.bools)
        msgs = [self.message(i, b) for i in range(R) for b in range(4)] + list(self.bools)
        fresh = O.encrypt_blocks(msgs, seed=self.seed)
        return np.concatenate([fresh, O.trivial_blocks([self.message(R + B, b) for b in range(4)])])

    # -- (a) the device's gate array
    def upload(self, ctx, rows):
        R, B = len(self.radix), len(self.bools)
        hs = ctx.upload_radix(rows[:4 * R])
        hs += ctx.upload_bool(rows[4 * R:4 * R + B])
        return hs + [ctx.trivial(self.triv)]

    def fr_gates(self, handles):
        out = []
        for g in self.gates:
            fg = F.Gate()
            fg.n_in, fg.offset, fg.kind = len(g.ins), g.offset, g.kind
            for q, (src, w) in enumerate(g.ins):
                if src[0] == "g":
                    fg.in_[q], fg.in_block[q] = GATE_REF | src[1], 0
                else:
                    fg.in_[q], fg.in_block[q] = handles[src[1]], src[2]
                fg.in_w[q] = w
            for t in range(16):
                fg.lut[t] = g.lut[t]
            out.append(fg)
        return out

    # -- (b) the oracle's jobs: the executor's merge rule
    def signature(self, g):
        """ordered (input, weight) list after the trivial inputs are dropped, and the
        offset with them folded in"""
        key, off = [], g.offset
        for src, w in g.ins:
            if self.is_triv(src):
                off += 2 * w * self.plain(src)
            else:
                key.append((src, w))
        return tuple(key), off

    def jobs(self):
        """[level][job]: sign gates alone; a LUT of norm^2 <= 8 joins the open job of its
        signature while that has < 8 outputs, else opens one; other LUTs run direct; a job
        with one output is direct.  Jobs stand in the order of their first gate."""
        by_level = {}
        for gi, g in enumerate(self.gates):
            by_level.setdefault(g.level, []).append(gi)
        out = []
        for l in sorted(by_level):
            jl, open_job = [], {}
            for gi in by_level[l]:
                g = self.gates[gi]
                if g.kind == SIGN:
                    jl.append(Job([gi], JSIGN))
                    continue
                if norm2(g.lut) <= MV_MAX_NORM2:
                    sig = self.signature(g)
                    j = open_job.get(sig)
                    if j is not None and len(j.gates) < MAX_OUT:
                        j.gates.append(gi)
                        j.kind = MULTI
                        continue
                    open_job[sig] = j = Job([gi], DIRECT)
                    jl.append(j)
                    continue
                jl.append(Job([gi], DIRECT))
            out.append(jl)
        return out

    def oracle_job(self, job, kind=None, gates=None):
        """Oracle.gates job over the slot array [content rows, then one row per gate]"""
        gs = [self.gates[gi] for gi in (job.gates if gates is None else gates)]
        g0 = gs[0]
        ins = [((self.row(src[1], src[2]) if src[0] == "c" else self.n_rows + src[1]), w) for src, w in g0.ins]
        return (ins, g0.offset, [list(g.lut) for g in gs], job.kind if kind is None else kind)

    def oracle_eval(self, O, rows) -> np.ndarray:
        """every gate's output row, evaluated level by level (as Oracle.run_schedule does)"""
        slots = np.zeros((self.n_rows + len(self.gates), O.big + 1), dtype=np.uint64)
        slots[:self.n_rows] = rows
        for jl in self.jobs():
            outs = O.gates([self.oracle_job(j) for j in jl], slots)
            k = 0
            for j in jl:
                for gi in j.gates:
                    slots[self.n_rows + gi] = outs[k]
                    k += 1
        return slots[self.n_rows:]

    # -- (c) plaintext: Gate.s and Gate.value
    def check_plain(self):
        """s and the value of every gate, recomputed from the gates alone"""
        for gi, g in enumerate(self.gates):
            s2 = (g.offset + 2 * sum(w * self.plain(src) for src, w in g.ins)) % 64  # 2 s mod 64
            if g.kind == LUT:
                assert s2 % 2 == 0 and s2 // 2 < 16 and s2 // 2 == g.s and g.value == g.lut[s2 // 2], gi
            else:
                s = (s2 - 64 if s2 >= 32 else s2) / 2
                assert s2 % 2 == 1 and s == g.s and g.value == int(s > 0), gi

    def level1(self) -> "Program":
        """the program cut to its first level (level-1 gates come first)"""
        n = sum(g.level == 1 for g in self.gates)
        assert all(g.level == 1 for g in self.gates[:n])
        return Program(self.name + "-level1", self.seed, self.radix, self.bools, self.triv, self.gates[:n])


# ------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self, prog: Program, rng: random.Random):
        self.p, self.rng = prog, rng
        self.used = set()      # (level, (input, weight) list) of every LUT gate so far
        self.n_lut = 0
        self.n_sign = {True: 0, False: 0}
        self.window(0)

    def window(self, r):
        """repeat r works on its own four radix inputs and three booleans"""
        R = len(self.p.radix)
        self.blocks = [("c", 4 * r + i, b) for i in range(4) for b in range(4)]
        self.bits = [("c", R + 3 * r + i, 0) for i in range(3)]
        self.handle0 = 4 * r
        self.triv = [("c", self.p.triv_input, b) for b in range(4)]

    def emit(self, g):
        self.p.gates.append(g)
        return len(self.p.gates) - 1

    def sigma(self, ins):
        return sum(w * self.p.plain(src) for src, w in ins)

    def w1(self):
        return self.rng.choice([w for w in range(-128, 128) if w])

    def draw(self, n, srcs=None, triv=False):
        """n fresh inputs on distinct blocks, and with triv a block of the trivial radix among them"""
        pick = self.rng.sample((self.blocks + self.bits) if srcs is None else srcs, n)
        ins = [(s, self.w1()) for s in pick]
        if triv:
            ins.insert(self.rng.randrange(len(ins) + 1), (self.rng.choice(self.triv), self.w1()))
        return ins

    def lut_gates(self, ins, luts, level=1, tag="", redraw=None):
        """LUT gates sharing one input list and offset; the offset comes last, so that
        s = offset/2 + sum w m (mod 32) lands on a chosen value of [0, 16), and is
        negative, zero and positive in turn (zero: s is the sum itself, inputs redrawn
        until that lies in [0, 16))"""
        mode = self.n_lut % 3
        target = [0, 15, 7, 8][self.n_lut] if self.n_lut < 4 else self.rng.randrange(16)
        self.n_lut += 1
        if mode == 1:
            while redraw is not None and self.sigma(ins) % 32 >= 16:
                ins = redraw()
            if self.sigma(ins) % 32 < 16:
                target = self.sigma(ins) % 32
        off = 2 * ((target - self.sigma(ins)) % 32)
        if mode == 0:
            off -= 64
        elif mode == 2 and off == 0:
            off += 64
        self.used.add((level, tuple(ins)))
        return [Gate(list(ins), off, LUT, list(l), level, target, l[target], tag) for l in luts]

    def sign_gate(self, ins, positive, level=1, tag=""):
        """s a non-zero half-integer on the chosen side of zero, next to zero and next
        to +-16 in turn"""
        k = self.n_sign[positive]
        self.n_sign[positive] += 1
        mag = [1, 31, 7, 15][k] if k < 4 else self.rng.randrange(1, 32, 2)
        s2 = mag if positive else -mag  # 2 s
        off = (s2 - 2 * self.sigma(ins)) % 64
        if k % 2:
            off -= 64
        return Gate(list(ins), off, SIGN, [0] * 16, level, s2 / 2, int(positive), tag)

    def big_lut(self):
        while True:
            l = [self.rng.randrange(16) for _ in range(16)]
            if norm2(l) > MV_MAX_NORM2:
                return l

    def group(self, g, tag="", luts=None, triv=False, n_in=None):
        """g level-1 LUT gates of norm^2 <= 8 on one input list that no earlier gate has"""
        luts = self.rng.sample(SMALL_POOL, g) if luts is None else luts
        n = self.rng.randrange(1, 7) if n_in is None else n_in

        def redraw():
            while True:
                ins = self.draw(n, triv=triv)
                if (1, tuple(ins)) not in self.used:
                    return ins
        return self.lut_gates(redraw(), luts, 1, tag or "group%d" % g, redraw)

    def direct(self, ins, level=1, tag="direct"):
        return self.lut_gates(ins, [self.big_lut()], level, tag)[0]

    # the structure every repeat has: 44 level-1 jobs in a fixed order
    def core(self, rep):
        self.window(rep)
        e, rng, blocks = self.emit, self.rng, self.blocks
        ref = {}
        # jobs 0, 1: (multi x 8, sign)
        lu = SPECIAL + rng.sample(SMALL_POOL[4:], 4)
        ref["multi"] = [e(x) for x in self.group(8, luts=lu, triv=True, n_in=3, tag="group8-special")][2]
        ref["sign"] = e(self.sign_gate(self.draw(1), True, tag="sign1"))
        # jobs 2, 3: (sign, direct)
        e(self.sign_gate(self.draw(2), False, tag="sign2"))
        ref["direct"] = e(self.direct(self.draw(1), tag="nin1"))
        # jobs 4, 5: (direct, multi x 2); the direct gate reads one block twice, with two weights
        b = rng.choice(blocks)
        e(self.direct([(b, 5), (b, -3)], tag="nin2-block-twice"))
        for x in self.group(2):
            e(x)
        # jobs 6, 7: (multi x 3, multi x 4); then 5, 6, 7
        for g in (3, 4, 5, 6, 7):
            for x in self.group(g, triv=(g == 5)):
                e(x)
        # 9 gates: 8 + a direct one; 10: 8 + 2; 17: 8 + 8 + a direct one
        for g in (9, 10, 17):
            for x in self.group(g):
                e(x)
        # a group of 3 interleaved with unrelated gates: the constant gates (n_in = 0)
        a, b_, c = self.group(3, tag="group3-interleaved")
        e(a)
        e(self.lut_gates([], [self.big_lut()], tag="nin0-lut")[0])
        e(b_)
        e(self.sign_gate([], True, tag="nin0-sign"))
        e(c)
        # a group with a norm^2 = 10 LUT in its middle: that gate runs direct
        a, b_, c = self.group(3, luts=[rng.choice(SMALL_POOL[4:]), NORM10, ONES8], tag="group-norm10-middle")
        for x in (a, b_, c):
            e(x)
        # every n_in from 3 to 16 as a direct job
        for n in range(3, 17):
            if n == 3:
                ins = [(s, w) for s, w in zip(rng.sample(blocks, 3), (-128, 127, 0))]
                tag = "nin3-extreme-weights"
            elif n == 4:
                ins = [(("c", self.handle0, blk), self.w1()) for blk in range(4)]
                tag = "nin4-one-handle-four-blocks"
            elif n == 16:
                ins = self.draw(16, blocks)  # all four blocks of all four handles
                ins[0] = (ins[0][0], -128)
                ins[15] = (ins[15][0], 127)
                tag = "nin16"
            else:  # n fresh inputs; two of the gates read the trivial radix as well
                ins = self.draw(n, triv=(n in (7, 12)))
                tag = "nin%d" % n + ("-triv" if n in (7, 12) else "")
            e(self.direct(ins, tag=tag))
        # sign gates: fan-in 1, 2, 15, 16 on both sides of zero, one with no input
        e(self.sign_gate(self.draw(1), False, tag="sign1"))
        e(self.sign_gate(self.draw(2, triv=True), True, tag="sign2-triv"))
        for n in (15, 16):
            for pos in (True, False):
                e(self.sign_gate(self.draw(n), pos, tag="sign%d" % n))
        e(self.sign_gate([], False, tag="nin0-sign"))
        return ref

    W2 = (1, -1, 2, -2)  # level 2: small weights, so that the summed bootstrap noise stays small

    def l2_ins(self, ref, n_content=1, triv=False):
        ins = [(("g", ref[k]), self.rng.choice(self.W2)) for k in ("multi", "sign", "direct")]
        ins += [(s, self.rng.choice(self.W2)) for s in self.rng.sample(self.blocks + self.bits, n_content)]
        if triv:
            ins.append((self.rng.choice(self.triv), self.rng.choice(self.W2)))
        self.rng.shuffle(ins)
        return ins

    def l2_single(self, ref):
        """one level-2 job: multi x 4 on three level-1 outputs, a content block and the trivial radix"""
        ins = self.l2_ins(ref, triv=True)
        for x in self.lut_gates(ins, self.rng.sample(SMALL_POOL, 4), 2, "l2-group4", lambda: self.l2_ins(ref, triv=True)):
            self.emit(x)

    def l2_mix(self, ref):
        """(multi x 8, sign), (direct, multi x 2), sign on level-1 outputs and content inputs"""
        e = self.emit
        for x in self.lut_gates(self.l2_ins(ref), self.rng.sample(SMALL_POOL, 8), 2, "l2-group8", lambda: self.l2_ins(ref)):
            e(x)
        e(self.sign_gate(self.l2_ins(ref, 0), True, 2, "l2-sign"))
        e(self.direct(self.l2_ins(ref, 2), 2, "l2-direct"))
        for x in self.lut_gates(self.l2_ins(ref, 2, True), self.rng.sample(SMALL_POOL, 2), 2, "l2-group2",
                                lambda: self.l2_ins(ref, 2, True)):
            e(x)
        e(self.sign_gate(self.l2_ins(ref, 1, True), False, 2, "l2-sign"))


SMALL_SEED, LARGE_SEED, LARGE_REPEATS = 11, 12, 6


def build(name: str, seed: int | None = None) -> Program:
    """"small": one core (44 level-1 jobs, one level-2 job).  "large": six cores on
    further inputs and a closing multi x 8 job (265 level-1 jobs), 30 level-2 jobs."""
    reps = {"small": 1, "large": LARGE_REPEATS}[name]
    seed = {"small": SMALL_SEED, "large": LARGE_SEED}[name] if seed is None else seed
    rng = random.Random(seed)
    p = Program(name, seed, [rng.randrange(256) for _ in range(4 * reps)], [rng.randrange(2) for _ in range(3 * reps)],
                rng.randrange(1, 256) | 0x41)
    b = _Builder(p, rng)
    refs = [b.core(r) for r in range(reps)]
    if name == "large":
        b.window(0)
        for x in b.group(8, tag="group8-tail"):
            b.emit(x)
    for r, ref in enumerate(refs):
        b.window(r)
        if name == "small":
            b.l2_single(ref)
        else:
            b.l2_mix(ref)
    return p


# ------------------------------------------------------- blind-rotation edge rows
def edge_rows(n: int, N: int, seed: int = 5):
    """(names, keyswitched rows (U, n+1), direct LUTs (U, 16)): mask and body words at
    the edges of the step-skip logic.  With L = log2(2N), a word v << (64-L) switches
    to a = v; 2^64-1 and 2^64 - 2^(63-L) to 2N = 0 (non-zero words, idle steps);
    2^64 - 2^(63-L) - 1 to 2N-1; a tie (v << (64-L)) + 2^(63-L) rounds up to v+1, the
    word below it to v."""
    rng = np.random.default_rng(seed)
    L = (2 * N).bit_length() - 1
    sh = 64 - L
    steps = n // 2
    assert n % 2 == 0
    word = lambda v: np.uint64((int(v) % (2 * N)) << sh)
    FULL, WRAP2, TOP = np.uint64(2**64 - 1), np.uint64(2**64 - 2**(sh - 1)), np.uint64(2**64 - 2**(sh - 1) - 1)
    rand = lambda size=None: rng.integers(0, 2**64 - 1, size, dtype=np.uint64, endpoint=True)
    names, rows = [], []

    def add(name, mask, body=None):
        r = np.zeros(n + 1, dtype=np.uint64)
        r[:n] = mask
        r[n] = rand() if body is None else body
        names.append(name)
        rows.append(r)

    z = lambda: np.zeros(n, dtype=np.uint64)
    add("zero", z())
    add("wrap", np.full(n, FULL))
    m = np.full(n, FULL); m[1::3] = WRAP2; m[2::3] = 0
    add("wrap-mixed", m)
    for name, idx in (("pair0", [0, 1]), ("pair370", [n - 2, n - 1]), ("coef0", [0]), ("coef741", [n - 1])):
        m = z(); m[idx] = rand(len(idx))
        add(name, m)
    busy = rand(n).reshape(steps, 2)
    m = busy.copy(); m[0::2] = 0
    add("even-idle", m.reshape(n))
    m = busy.copy(); m[1::2] = 0
    add("odd-idle", m.reshape(n))
    m = np.zeros((steps, 2), dtype=np.uint64)
    t, run = 0, 1
    while t < steps:  # a busy step, then idle runs of growing length
        m[t] = rand(2)
        t += 1 + run
        run += 1
    add("idle-runs", m.reshape(n))
    add("all-N", np.full(n, word(N)))
    v = rng.integers(1, 2 * N, steps)
    add("sum-0", np.stack([[word(x), word(2 * N - x)] for x in v]).reshape(n))
    add("sum-N", np.stack([[word(x), word(N - x)] for x in v]).reshape(n))
    add("alt-v0", np.stack([[word(x), 0] if t % 2 else [0, word(x)] for t, x in enumerate(v)]).astype(np.uint64).reshape(n))
    m = z(); m[0::2] = word(1); m[1::2] = TOP
    add("alt-1-top", m)
    tie = np.array([(int(x) << sh) + 2**(sh - 1) for x in rng.integers(0, 2 * N - 1, n)], dtype=np.uint64)
    tie[1::3] -= np.uint64(1)  # the word below a tie: rounds down
    tie[2::3] += np.uint64(1)
    add("ties", tie)
    for b in (0, 1, N // 32 - 1, N // 32, N - 1, N, N + N // 32, 2 * N - 1):  # bodies on LUT box boundaries
        add("body-%d" % b, rand(n), word(b))
    add("body-wrap", rand(n), FULL)
    add("random0", rand(n))
    add("random1", rand(n))
    luts = rng.integers(0, 16, (len(rows), 16), dtype=np.uint8)
    luts[0] = np.arange(16)
    return names, np.stack(rows), luts


EDGE_HEAD = [("zero", "wrap"), ("zero", "random0"), ("pair0", "pair370"), ("pair370", "pair370"),
             ("even-idle", "odd-idle"), ("even-idle", "even-idle")]


def edge_order(names, count: int):
    """row indices of a launch of `count` (odd) bootstraps: the workgroup pairs of
    EDGE_HEAD, the unique rows repeated, the all-zero row alone at the end"""
    assert count % 2 == 1 and count > 2 * len(EDGE_HEAD)
    at = {nm: i for i, nm in enumerate(names)}
    order = [at[x] for pr in EDGE_HEAD for x in pr]
    u = 0
    while len(order) < count - 1:
        order.append(u % len(names))
        u += 1
    return order + [at["zero"]]
