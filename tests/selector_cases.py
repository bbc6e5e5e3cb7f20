"""Inputs and oracle evaluations shared by the selector tests (tests/test_selector_oracle.py on
the CPU, tests/test_private_needle_gpu.py and tests/test_find_clear_gpu.py on the device).  No
GPU use, no test functions; tests/gate_programs.py is the precedent.

A selector job's rotation starts from a GLWE [k + 1][N] of uniform 64-bit words, which the f64
ladder converts with (double)(int64_t): PLANTED are the words at that conversion's edges."""
import numpy as np

import fheregex as F
from test_find_clear import extract_sum

U = np.uint64
# 0 and 1; 2^63 - 1 rounds up to 2^63, which wraps to -2^63; -2^63 itself; 2^63 + 1 = -(2^63 - 1)
# rounds down to it; 2^64 - 1 = -1 changes sign; 2^53 + 1 is a tie (to even: 2^53)
PLANTED = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 53 + 1]


def random_accs(count, k, N, seed):
    """uniform-random GLWEs [count][k + 1][N] with the PLANTED words at random places of every
    polynomial"""
    rng = np.random.default_rng(seed)
    acc = rng.integers(0, 2 ** 64 - 1, (count, k + 1, N), dtype=U, endpoint=True)
    for q in range(count):
        for c in range(k + 1):
            acc[q, c, rng.choice(N, len(PLANTED), replace=False)] = np.array(PLANTED, dtype=U)
    return acc


def balanced_chunks(m):
    """lower.h for_balanced_chunks: ceil(m / 16) contiguous chunks, the longer ones first"""
    chunks = (m + 15) // 16
    out, start = [], 0
    for c in range(chunks):
        ln = m // chunks + (1 if c < m % chunks else 0)
        out.append((start, ln))
        start += ln
    return out


def find_clear_values(S, sel, text: bytes, m):
    """{gate: LWE} of a find_clear schedule's extract-sums (over every start of the text): start
    by start, chunk by chunk of the 2 m tests, term t = (selector t, position p + t // 2, half
    t % 2) (lower.cpp compile_needle_over); the gates are the level-1 jobs' single inputs, in
    order"""
    lvl1 = S.jobs[:S.level_off[1]] if len(S.level_off) > 1 else []
    gates = [j.in_ref[0] for j in lvl1]
    sums = [[(t, p + t // 2, t % 2) for t in range(first, first + ln)]
            for p in range(len(text) - m + 1) for first, ln in balanced_chunks(2 * m)]
    assert len(sums) == len(gates) == len(set(gates))
    return {g: extract_sum(sel, text, terms) for g, terms in zip(gates, sums)}


def oracle_find(O, sel, m, content_lwes=None, text=None, starts=False):
    """the LWE of every output of fr_find / fr_find_starts (content_lwes: [n][4][kN + 1]) or of
    fr_find_clear / fr_find_clear_starts (text: the clear bytes) under the oracle, from the
    needle's selectors sel [2 m][k + 1][N]"""
    if text is None:
        S = F.schedule_find(len(content_lwes), m, starts=starts)
        O.run_schedule(S, content_lwes, selectors=sel)
    else:
        S = F.schedule_find_clear(len(text), m, starts=starts)
        O.run_schedule(S, None, values=find_clear_values(S, sel, text, m))
    return np.stack([O._output(*p) for p in S.parts])
