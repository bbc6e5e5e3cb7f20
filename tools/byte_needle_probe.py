"""Byte-table needles on one MI355X: what a search over clear content costs with a byte-table
needle next to the nibble needle of the same literal, on the same box in the same run.

find_clear, find_clear_starts and scan_clear over n_chars (default 256) clear characters for
literal needles of m = 3, 8 and 16, once with the nibble form and once with the byte form of the
same literal, every plan cached: host clock around each blocking call (fr_set_async(0)),
alternating, `reps` of each (default 20); the rotation counts of each; both blob sizes; and the
extract-sum kernel's own HIP-event time for the sums find_clear_starts launches in each form.
At m <= 8 both forms run the same rotations (one per start); at m = 16 the byte form runs one per
start where the nibble form runs two chunk gates and an AND.
One JSON line, also written to the output path (default profiles/byte_needle/byte_needle_probe_k<k>.json).
Usage: python3 tools/byte_needle_probe.py [reps] [n_chars] [out_path]; BYTE_NEEDLE_PROBE_K=2: (2, 1024)"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
import fheregex as F  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_chars = int(sys.argv[2]) if len(sys.argv) > 2 else 256
k = int(os.environ.get("BYTE_NEEDLE_PROBE_K", "1"))
N = 2048 if k == 1 else 1024
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(REPO, "profiles", "byte_needle",
                                                              "byte_needle_probe_k%d.json" % k)


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0, params=F.default_params(k=k, N=N, ring=F.RING_FFT))
ctx.load_client_key(blob)
ctx.gen_server_key(42)
res = {"device": ctx.info(), "k": k, "N": N, "reps": reps, "n_chars": n_chars,
       "env": {a: v for a, v in os.environ.items() if a.startswith("FR_")}}

text = ("xyabcz" * (n_chars // 6 + 1))[:n_chars]
ctx.set_async(False)
literals = {3: "abc", 8: "abczxyab", 16: "abczxyabczxyabcz"}
FORMS = ("nibbles", "bytes")
nd, sizes = {}, {}
for m, s in literals.items():
    blobs = {"nibbles": ctx.encrypt_needle(F.needle_masks(s), seed=7),
             "bytes": ctx.encrypt_needle_bytes(F.needle_tables(s), seed=7)}
    sizes["m%d" % m] = {form: len(b) for form, b in blobs.items()}
    for form, b in blobs.items():
        nd[m, form] = ctx.upload_needle(b)
        assert nd[m, form].form == (F.NEEDLE_BYTES if form == "bytes" else F.NEEDLE_NIBBLES)
res["blob_bytes"] = sizes


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
for m in literals:
    for form in FORMS:
        paths["find_clear_m%d_%s" % (m, form)] = lambda m=m, form=form: one(ctx.find_clear, text, nd[m, form])
        paths["find_clear_starts_m%d_%s" % (m, form)] = lambda m=m, form=form: many(ctx.find_clear_starts, text,
                                                                                    nd[m, form])
        paths["scan_clear_m%d_%s" % (m, form)] = lambda m=m, form=form: one(ctx.scan_clear, text, nd[m, form])
ctx.set_plan_cache(len(paths))
stats = {}
for _ in range(2):  # warm-up: every plan cached
    for name, f in paths.items():
        stats[name] = f()
# the answers, once: both forms against the plaintext evaluations
for m, s in literals.items():
    want = F.plain_find_clear(text, F.needle_masks(s))
    assert want == F.plain_find_clear_bytes(text, F.needle_tables(s)) and want[1] == 1
    for form in FORMS:
        hs = ctx.find_clear_starts(text, nd[m, form])
        assert [ctx.decrypt_radix(ctx.download_radix(h)) for h in hs] == want[0], (m, form)
        drop(hs)
ms = {name: [] for name in paths}
for r in range(reps):
    for name, f in paths.items():
        t = time.perf_counter()
        st = f()
        ms[name].append((time.perf_counter() - t) * 1e3)
        assert st.plan_cached == 1
res["host_clock_ms"] = {name: stat(v) for name, v in ms.items()}
res["rotations"] = {name: {"pbs": int(st.pbs), "rotations": int(st.blind_rotations), "levels": int(st.levels),
                           "max_level_width": int(st.max_level_width)} for name, st in stats.items()}
ratios = {}
for m in literals:
    for kind in ("find_clear", "find_clear_starts", "scan_clear"):
        a = res["host_clock_ms"]["%s_m%d_nibbles" % (kind, m)]["median"]
        b = res["host_clock_ms"]["%s_m%d_bytes" % (kind, m)]["median"]
        ratios["%s_m%d" % (kind, m)] = round(b / a, 3)
res["bytes_over_nibbles"] = ratios

# the kernel alone: the sums find_clear_starts launches, in each form
ctx.set_profiling(1)
kernel = {}
for m in literals:
    for form in FORMS:
        if form == "bytes":
            chunks = [(0, m)] if m <= 16 else None
            sums = [[(t, p + t, 0) for t in range(a, a + ln)] for p in range(n_chars - m + 1) for a, ln in chunks]
        else:
            chunks = [(0, 2 * m)] if 2 * m <= 16 else [(0, m), (m, m)]
            sums = [[(t, p + t // 2, t % 2) for t in range(a, a + ln)] for p in range(n_chars - m + 1)
                    for a, ln in chunks]
        ctx.dev_select_sum(nd[m, form], text, sums)  # warm-up
        t_ms = []
        for r in range(reps):
            ctx.dev_select_sum(nd[m, form], text, sums)
            t_ms.append(ctx.select_sum_timer())
        s = stat(t_ms)
        s["sums"], s["terms"] = len(sums), len(sums[0])
        kernel["m%d_%s" % (m, form)] = s
ctx.set_profiling(0)
res["select_sum_kernel_ms"] = kernel
for n_ in nd.values():
    n_.close()
line = json.dumps(res)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
