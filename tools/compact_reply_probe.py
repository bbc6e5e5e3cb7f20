"""The compact reply on one MI355X: what the one call from match to blob costs and saves.

/abc/ over 256 encrypted characters at (k, N) = (1, 2048), the plan cached, one process.  After
a warm-up of every path, `reps` repetitions (default 9), the paths alternating within a
repetition, a host clock around each (every path ends in its own synchronised download):
  - two_step: fr_match_starts + fr_pack_bools_blob + the release of the 256 handles;
  - packed_full / packed_compact: fr_match_starts_packed in the FRPKRES1 and FRCPRES1 forms.
Then, in a pass of their own under fr_set_profiling, the HIP-event ms of the pack's stages
(digits, int8 GEMM, rotate-sum, and the compact form's rounding kernel) of both forms.
Medians and ranges, the reply sizes, and whether the ranges overlap; one JSON line.
Usage: python3 tools/compact_reply_probe.py [reps] [n_chars]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
import fheregex as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
n_chars = int(sys.argv[2]) if len(sys.argv) > 2 else 256
PATTERN = "/abc/"


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0)
ctx.load_client_key(blob)
ctx.gen_server_key(42)
ctx.gen_packing_key(7)
text = ("xyabcz" * (n_chars // 6 + 1))[:n_chars]
chars = ctx.upload_radix(ctx.encrypt_str(text, seed=1))
want = F.plain_match_starts(text, PATTERN)[1]


def two_step():
    hs = ctx.match_starts(chars, PATTERN)
    reply = ctx.pack_bools(hs)
    for h in hs:
        ctx.release(h)
    return reply


def packed_full():
    return ctx.match_starts_packed(chars, PATTERN, compact=False)


def packed_compact():
    return ctx.match_starts_packed(chars, PATTERN, compact=True)


paths = {"two_step": two_step, "packed_full": packed_full, "packed_compact": packed_compact}
replies = {}
for _ in range(2):  # warm-up: the plan, the scratch of every path
    for name, f in paths.items():
        replies[name] = f()
assert replies["two_step"] == replies["packed_full"]
assert ctx.decrypt_packed(replies["packed_full"]) == want == ctx.decrypt_packed_compact(replies["packed_compact"])

ms = {name: [] for name in paths}
for r in range(reps):
    for name, f in paths.items():
        t = time.perf_counter()
        f()
        ms[name].append((time.perf_counter() - t) * 1e3)

res = {"device": ctx.info(), "reps": reps, "n_chars": n_chars, "pattern": PATTERN,
       "env": {k: v for k, v in os.environ.items() if k.startswith("FR_")},
       "host_clock_ms": {name: stat(v) for name, v in ms.items()},
       "reply_bytes": {name: len(v) for name, v in replies.items()}}
a = res["host_clock_ms"]["two_step"]
for name in ("packed_full", "packed_compact"):
    b = res["host_clock_ms"][name]
    res[name + "_vs_two_step"] = {"median_ratio": round(b["median"] / a["median"], 4),
                                  "ranges_overlap": b["max"] >= a["min"] and a["max"] >= b["min"]}

ctx.set_profiling(1)
stages = {"packed_full": [], "packed_compact": []}
for r in range(reps):
    for name in stages:
        paths[name]()
        stages[name].append(ctx.pack_timers_compact())
for name, v in stages.items():
    res[name + "_stage_ms"] = {s: stat([x[i] for x in v])
                               for i, s in enumerate(("digits", "gemm", "rotate_sum", "compress"))}
print(json.dumps(res), flush=True)
