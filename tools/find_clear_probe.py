"""Private search over clear content on one MI355X: what a find costs when the server holds the
text itself, next to the same find on an encryption of that text, and the extract-sum kernel alone.

(a) search: find_clear and find_clear_starts for needles of m = 3 and m = 8 over n_chars (default
    256) clear characters, next to find and find_starts on an encryption of the same text, every
    plan cached: host clock around each blocking call (fr_set_async(0)), alternating, `reps` of
    each (default 20), and the rotation counts of each.
(b) kernel: fr_dev_select_sum under fr_set_profiling, the kernel's own HIP-event time, for the
    sums those finds launch (n_chars - m + 1 sums of 2 m terms) and for m = 8 over 4,096
    characters (4,089 sums of 16 terms), with the bytes it writes (sums x (k N + 1) x 8) over
    that time.  The hook's staging and download are outside the events.
One JSON line, also written to the output path (default profiles/find_clear/find_clear_probe_k<k>.json).
Usage: python3 tools/find_clear_probe.py [reps] [n_chars] [out_path]; FIND_CLEAR_PROBE_K=2: (2, 1024)"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
import fheregex as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_chars = int(sys.argv[2]) if len(sys.argv) > 2 else 256
k = int(os.environ.get("FIND_CLEAR_PROBE_K", "1"))
N = 2048 if k == 1 else 1024
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "find_clear",
                                                              "find_clear_probe_k%d.json" % k)


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0, params=F.default_params(k=k, N=N, ring=F.RING_FFT))
ctx.load_client_key(blob)
ctx.gen_server_key(42)
res = {"device": ctx.info(), "k": k, "N": N, "reps": reps, "n_chars": n_chars,
       "env": {a: v for a, v in os.environ.items() if a.startswith("FR_")}}

# ---- (a) the search
text = ("xyabcz" * (n_chars // 6 + 1))[:n_chars]
chars = ctx.upload_radix(ctx.encrypt_str(text, seed=1))
ctx.set_async(False)
needles = {3: "abc", 8: "abczxyab"}
nd = {m: ctx.upload_needle(ctx.encrypt_needle(F.needle_masks(s), seed=7)) for m, s in needles.items()}


def drop(hs):
    for h in hs:
        ctx.release(h)


def one(fn, *args):
    out, st = fn(*args)
    drop([out])
    return st


def many(fn, *args):
    outs, st = fn(*args, stats=True)
    drop(outs)
    return st


paths = {}
for m in needles:
    paths["find_clear_m%d" % m] = lambda m=m: one(ctx.find_clear, text, nd[m])
    paths["find_m%d" % m] = lambda m=m: one(ctx.find, chars, nd[m])
    paths["find_clear_starts_m%d" % m] = lambda m=m: many(ctx.find_clear_starts, text, nd[m])
    paths["find_starts_m%d" % m] = lambda m=m: many(ctx.find_starts, chars, nd[m])
ctx.set_plan_cache(len(paths))
stats = {}
for _ in range(2):  # warm-up: every plan cached
    for name, f in paths.items():
        stats[name] = f()
# the answers, once: both finds against the plaintext evaluation
for m, s in needles.items():
    want = F.plain_find_clear(text, F.needle_masks(s))
    a = ctx.find_clear_starts(text, nd[m])
    b = ctx.find_starts(chars, nd[m])
    assert [ctx.decrypt_radix(ctx.download_radix(h)) for h in a] == want[0]
    assert [ctx.decrypt_radix(ctx.download_radix(h)) for h in b] == want[0] and want[1] == 1
    drop(a + b)
ms = {name: [] for name in paths}
for r in range(reps):
    for name, f in paths.items():
        t = time.perf_counter()
        st = f()
        ms[name].append((time.perf_counter() - t) * 1e3)
        assert st.plan_cached == 1
res["search_host_clock_ms"] = {name: stat(v) for name, v in ms.items()}
res["search_rotations"] = {name: {"pbs": int(st.pbs), "rotations": int(st.blind_rotations), "levels": int(st.levels),
                                  "max_level_width": int(st.max_level_width)} for name, st in stats.items()}
for m in needles:
    for kind in ("", "_starts"):
        a = res["search_host_clock_ms"]["find_clear%s_m%d" % (kind, m)]["median"]
        b = res["search_host_clock_ms"]["find%s_m%d" % (kind, m)]["median"]
        res["search_host_clock_ms"]["find%s_over_find_clear%s_m%d" % (kind, kind, m)] = round(b / a, 3)

# ---- (b) the kernel alone
ctx.set_profiling(1)
kernel = {}
for m, n in ((3, n_chars), (8, n_chars), (8, 4096)):
    body = bytes(np.random.default_rng(n + m).integers(0, 256, n, dtype=np.uint8))
    sums = [[(t, p + t // 2, t % 2) for t in range(2 * m)] for p in range(n - m + 1)]
    ctx.dev_select_sum(nd[m], body, sums)  # warm-up
    t_ms = []
    for r in range(reps):
        ctx.dev_select_sum(nd[m], body, sums)
        t_ms.append(ctx.select_sum_timer())
    s = stat(t_ms)
    s["sums"], s["terms"] = len(sums), 2 * m
    s["bytes_written"] = len(sums) * (k * N + 1) * 8
    s["write_GB_per_s_at_median"] = round(s["bytes_written"] / (s["median"] * 1e-3) / 1e9, 1)
    kernel["m%d_n%d" % (m, n)] = s
ctx.set_profiling(0)
res["select_sum_kernel_ms"] = kernel
for n_ in nd.values():
    n_.close()
line = json.dumps(res)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
