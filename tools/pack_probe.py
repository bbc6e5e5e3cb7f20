"""Packed results on one MI355X: what a packed reply costs and saves.

For n = 16, 256, 2048 booleans (real bootstrap-shaped LWEs: uploaded encryptions), 7
repetitions after a warm-up, the two ways of returning them alternating within a repetition:
  - HIP-event ms of the pack's three stages (fr_set_profiling: digits, int8 GEMM, rotate-sum);
  - host clock around pack_bools (launch + download of the one GLWE), against the host clock
    around downloading the same n booleans one by one (fr_download_radix, the existing way);
  - the bytes of each reply.
Then k_gen_pksk + limb build (gen_packing_key), the key's load (load_packing_key of the
exported blob) and, as the GEMM's yardstick, the LWE keyswitch at the same row counts
(dev_bench_pbs total - blind rotation, as tools/ks_probe.py).  Medians and ranges, one JSON line.
Usage: python3 tools/pack_probe.py [reps] [sizes...]   (FR_PK_SPLIT / FR_KS_* for A/B runs)"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
import fheregex as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
sizes = [int(x) for x in sys.argv[2:]] or [16, 256, 2048]


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0)
ctx.load_client_key(blob)
ctx.gen_server_key(42)
res = {"device": ctx.info(), "reps": reps, "env": {k: v for k, v in os.environ.items() if k.startswith("FR_")}}

gen, load = [], []
for r in range(reps + 1):
    t = time.perf_counter()
    ctx.gen_packing_key(7)
    gen.append((time.perf_counter() - t) * 1e3)
key = ctx.export_packing_key()
for r in range(reps + 1):
    t = time.perf_counter()
    ctx.load_packing_key(key)
    load.append((time.perf_counter() - t) * 1e3)
res["gen_packing_key_ms"] = stat(gen[1:])   # host noise draws + k_gen_pksk + limbs, host clock
res["load_packing_key_ms"] = stat(load[1:])  # H2D of the rows + limbs, host clock
res["packing_key_bytes"] = len(key)
del key

ctx.set_profiling(1)
hs = ctx.upload_bool(ctx.encrypt_blocks([i % 2 for i in range(max(sizes))], seed=3).reshape(max(sizes), -1))
res["sizes"] = {}
for n in sizes:
    batch = hs[:n]
    ctx.pack_bools(batch)
    for h in batch[:4]:
        ctx.download_radix(h)
    stages, pack, each = [], [], []
    for r in range(reps):
        t = time.perf_counter()
        reply = ctx.pack_bools(batch)
        pack.append((time.perf_counter() - t) * 1e3)
        stages.append(ctx.pack_timers())
        t = time.perf_counter()
        got = [ctx.download_radix(h)[0] for h in batch]
        each.append((time.perf_counter() - t) * 1e3)
    ks = []
    ksb = [hs[i % len(hs)] for i in range(n)]
    ctx.dev_bench_pbs(ksb, 1)
    for r in range(reps):
        br, tot = ctx.dev_bench_pbs(ksb, 1)
        ks.append(tot - br)
    res["sizes"][n] = {
        "digits_ms": stat([s[0] for s in stages]), "gemm_ms": stat([s[1] for s in stages]),
        "rotate_sum_ms": stat([s[2] for s in stages]), "pack_host_clock_ms": stat(pack),
        "download_each_host_clock_ms": stat(each), "packed_reply_bytes": len(reply),
        "separate_reply_bytes": n * got[0].nbytes, "lwe_keyswitch_ms": stat(ks),
        "gemm_yardstick_ms": round(statistics.median(ks) * (6144 * 4096) / (10240 * 743), 4),
    }
print(json.dumps(res), flush=True)
