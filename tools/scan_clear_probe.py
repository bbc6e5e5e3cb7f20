"""Scan of a long clear text on one MI355X: what a search costs at one rotation per distinct
window, next to find_clear's one rotation per start on the same text, and the mapped rotate-sum
next to k_pack_rotate_sum.

Texts are generated, never read from a file: a seeded synthetic log (lines built from small fixed
vocabularies by numpy.random.default_rng) and seeded uniform random bytes (the worst case: almost
every window distinct).
(a) 16,384 bytes of each text, m = 3 and 8: D, padded D, rotations and the host clock around each
    blocking call (fr_set_async(0), every plan cached, alternating, `reps` of each) of scan_clear
    and scan_clear_starts(compact) next to find_clear and ServerKey.find_clear_starts(compact);
    the two replies are compared byte for byte once.
(b) the scan alone on 1 MiB of the log.
(c) the pack's stages under fr_set_profiling for n = 256 and N starts: k_pack_rotate_sum (n rows)
    next to k_pack_map_sum over 64 rows and over n rows (the identity map).
One JSON line, also written to the output path (default profiles/scan_clear/scan_clear_probe_k<k>.json).
Usage: python3 tools/scan_clear_probe.py [reps] [out_path]; SCAN_CLEAR_PROBE_K=2: (2, 1024)"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
import fheregex as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
k = int(os.environ.get("SCAN_CLEAR_PROBE_K", "1"))
N = 2048 if k == 1 else 1024
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "scan_clear",
                                                              "scan_clear_probe_k%d.json" % k)
HOSTS = ["web-01", "web-02", "db-01", "cache-01", "queue-01", "auth-01"]
LEVELS = ["INFO", "INFO", "INFO", "WARN", "ERROR", "DEBUG"]
UNITS = ["nginx", "postgres", "redis", "worker", "sshd", "cron", "kernel"]
EVENTS = ["connection accepted from", "connection closed by", "request served in", "slow query took",
          "cache miss for key", "job finished with status", "session opened for user", "retrying after"]


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def synthetic_log(n, seed):
    rng = np.random.default_rng(seed)
    out, size, t = [], 0, 0
    while size < n:
        t += int(rng.integers(1, 90))
        line = "2025-03-%02d %02d:%02d:%02d %s %s[%d]: %s %s %d\n" % (
            1 + t // 86400 % 28, t // 3600 % 24, t // 60 % 60, t % 60, HOSTS[rng.integers(len(HOSTS))],
            UNITS[rng.integers(len(UNITS))], int(rng.integers(100, 400)), LEVELS[rng.integers(len(LEVELS))],
            EVENTS[rng.integers(len(EVENTS))], int(rng.integers(0, 1000)))
        out.append(line)
        size += len(line)
    return "".join(out).encode()[:n]


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0, params=F.default_params(k=k, N=N, ring=F.RING_FFT))
ctx.load_client_key(blob)
ctx.gen_server_key(42)
ctx.gen_packing_key(9, compact=True)
ck, sk = F.ClientKey(ctx), F.ServerKey(ctx)
ctx.set_async(False)
ctx.set_plan_cache(4)
res = {"device": ctx.info(), "k": k, "N": N, "reps": reps,
       "env": {a: v for a, v in os.environ.items() if a.startswith("FR_")}}


def timed(f, n):
    f()  # warm-up: the plan cached, the scratch grown
    ms, st = [], None
    for _ in range(n):
        t = time.perf_counter()
        st = f()
        ms.append((time.perf_counter() - t) * 1e3)
    return stat(ms), st


def scan_bool(text, nd):
    out, st = ctx.scan_clear(text, nd)
    ctx.release(out)
    return st


def find_bool(text, nd):
    out, st = ctx.find_clear(text, nd)
    ctx.release(out)
    return st


def rot(st):
    return {"rotations": int(st.blind_rotations), "levels": int(st.levels), "host_ms": round(st.host_ms, 3)}


def measure(text, with_find, n_reps):
    out = {"bytes": len(text)}
    for m in (3, 8):
        s = text[100:100 + m]
        masks = F.needle_masks(s)
        nd = sk.upload_needle(ctx.encrypt_needle(masks, seed=7))
        cls, D, Dpad, _ = F.window_classes(text, m)
        r = {"needle": s.decode("latin-1"), "D": D, "Dpad": Dpad, "starts_that_fit": len(text) - m + 1}
        ms, st = timed(lambda: scan_bool(text, nd), n_reps)
        r["scan_clear_ms"], r["scan_clear"] = ms, rot(st)
        ms, st = timed(lambda: ctx.scan_clear_starts(text, nd, compact=True, stats=True)[1], n_reps)
        r["scan_clear_starts_ms"], r["scan_clear_starts"] = ms, rot(st)
        reply = sk.scan_clear_starts(text, nd, compact=True)
        r["reply_bytes"] = len(reply)
        want = [p for p in range(len(text) - m + 1) if text.startswith(s, p)]
        assert ck.decrypt_starts(reply) == want and want
        if with_find:
            ms, st = timed(lambda: find_bool(text, nd), n_reps)
            r["find_clear_ms"], r["find_clear"] = ms, rot(st)
            ref = []
            ms, _ = timed(lambda: ref.append(sk.find_clear_starts(text, nd, compact=True)), n_reps)
            r["find_clear_starts_ms"] = ms
            r["find_clear_starts"] = {"rotations": len(F.schedule_find_clear(len(text), m, starts=True).jobs)}
            assert ref[-1] == reply  # byte for byte
        nd.close()
        out["m%d" % m] = r
    return out


res["log_16384"] = measure(synthetic_log(16384, 1), True, reps)
res["random_16384"] = measure(bytes(np.random.default_rng(2).integers(0, 256, 16384, dtype=np.uint8)), True, reps)
res["log_1MiB"] = measure(synthetic_log(1 << 20, 3), False, max(2, reps // 3))

# ---- (c) the rotate-sum stage, mapped and not
ctx.set_profiling(1)
hs = ctx.upload_bool(ctx.encrypt_blocks([i % 2 for i in range(N)], seed=3).reshape(N, -1))
stages = {}
for n in (256, N):
    def stage(f):
        f()
        t = []
        for _ in range(reps):
            f()
            t.append(ctx.pack_timers()[2])
        return stat(t)
    stages["n%d" % n] = {
        "rotate_sum_ms": stage(lambda: ctx.pack_bools(hs[:n])),
        "map_sum_64_rows_ms": stage(lambda: ctx.dev_pack_mapped(hs[:64], [j % 64 for j in range(n)])),
        "map_sum_identity_ms": stage(lambda: ctx.dev_pack_mapped(hs[:n], list(range(n)))),
    }
ctx.set_profiling(0)
res["pack_sum_stage_ms"] = stages
line = json.dumps(res)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
