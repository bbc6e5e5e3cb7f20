"""Private search on one MI355X: what a rotation from a ciphertext accumulator costs, and what
a find costs next to a has_match of the same literal.

(a) kernel: fr_dev_blind_rotate_acc (trivial selectors) against fr_dev_blind_rotate on the same
    keyswitched inputs, at 1, 254, 512 and 2,048 bootstraps, alternating, `reps` of each (default
    20), the launch's own HIP-event time (fr_set_profiling: the stamps of its dispatch); the LUT
    launch both bare and after H2D copies of the selector table's size into buffers that are
    then released (what surrounds the selector launch inside its hook).  At 1
    bootstrap the LUT launch takes the key-products path, which selector launches never take:
    run again with FR_FFT_KPRE_BATCH=0 for the like-for-like latency shape.
(b) search: find and find_starts for needles of m = 3 and m = 8 over n_chars (default 256)
    encrypted characters with the plan cached, next to has_match("/abc/") on the same content:
    host clock around each blocking call (fr_set_async(0)), alternating, and the rotation counts.
One JSON line.  Usage: python3 tools/needle_probe.py [reps] [n_chars]"""
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
k = int(os.environ.get("NEEDLE_PROBE_K", "1"))
N = 2048 if k == 1 else 1024


def stat(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
    blob = f.read()
ctx = F.Context(0, params=F.default_params(k=k, N=N, ring=F.RING_FFT))
ctx.load_client_key(blob)
ctx.gen_server_key(42)
res = {"device": ctx.info(), "k": k, "N": N, "reps": reps, "n_chars": n_chars,
       "env": {a: v for a, v in os.environ.items() if a.startswith("FR_")}}

# ---- (a) the kernel
rng = np.random.default_rng(5)
COUNTS = (1, 254, 512, 2048)
big = max(COUNTS)
ks64 = ctx.dev_keyswitch(ctx.encrypt_blocks(rng.integers(0, 16, 64), seed=6))
ks = np.tile(ks64, (big // 64, 1))
luts = rng.integers(0, 2, (big, 16), dtype=np.uint8)
mm = (np.arange(N) + N // 32) // (N // 16)
acc = np.zeros((big, k + 1, N), dtype=np.uint64)
for q in range(big):
    v = np.append(luts[q].astype(np.uint64) << np.uint64(59), np.uint64(-(int(luts[q][0]) << 59) % 2 ** 64))
    acc[q, k] = v[np.minimum(mm, 16)]


def br_ms(fn):
    t0 = ctx.device_timers()
    out = fn()
    t1 = ctx.device_timers()
    return t1["br_ms"] - t0["br_ms"], out


# The selector hook copies its table (n (k+1) N words) to the device right before its launch and
# the LUT hook copies nothing of that size, so `lut_after_copy` puts the same bytes on the bus
# before the LUT launch: needles of up to 64 characters (2 selectors each, one H2D copy per
# upload), uploaded and released.  The order within a repetition is lut, acc, lut_after_copy, so
# the bare LUT launch follows a LUT call, the selector launch a LUT call and its own allocation
# and copy, and lut_after_copy the selector hook's release and its own uploads and releases.
needle_blobs = {m: ctx.encrypt_needle([(1, 1)] * m, seed=8) for m in (1, 64)}


def copy_like_table(n):
    left = (n + 1) // 2  # characters whose selectors make n accumulators
    while left > 0:
        m = 64 if left >= 64 else 1
        ctx.upload_needle(needle_blobs[m]).close()
        left -= m


ctx.set_profiling(1)
kernel = {}
for n in COUNTS:
    lut_fn = lambda: ctx.dev_blind_rotate(ks[:n], luts[:n])  # noqa: E731
    acc_fn = lambda: ctx.dev_blind_rotate_acc(ks[:n], acc[:n])  # noqa: E731

    def lut_copy_fn():
        copy_like_table(n)
        return ctx.dev_blind_rotate(ks[:n], luts[:n])

    a, b, c = lut_fn(), acc_fn(), lut_copy_fn()  # warm-up, and the same words
    assert np.array_equal(a, b) and np.array_equal(a, c)
    ms = {"lut": [], "acc": [], "lut_after_copy": []}
    for r in range(reps):
        ms["lut"].append(br_ms(lut_fn)[0])
        ms["acc"].append(br_ms(acc_fn)[0])
        ms["lut_after_copy"].append(br_ms(lut_copy_fn)[0])
    s = {name: stat(v) for name, v in ms.items()}
    s["acc_over_lut_median"] = round(s["acc"]["median"] / s["lut"]["median"], 4)
    s["acc_over_lut_after_copy_median"] = round(s["acc"]["median"] / s["lut_after_copy"]["median"], 4)
    s["within_3_percent"] = s["acc"]["median"] <= 1.03 * s["lut"]["median"]
    s["within_3_percent_after_copy"] = s["acc"]["median"] <= 1.03 * s["lut_after_copy"]["median"]
    kernel[str(n)] = s
ctx.set_profiling(0)
res["kernel_br_ms"] = kernel

# ---- (b) the search
text = ("xyabcz" * (n_chars // 6 + 1))[:n_chars]
chars = ctx.upload_radix(ctx.encrypt_str(text, seed=1))
ctx.set_async(False)
needles = {3: "abc", 8: "abczxyab"}
nd = {m: ctx.upload_needle(ctx.encrypt_needle(F.needle_masks(s), seed=7)) for m, s in needles.items()}


def drop(hs_):
    for h in hs_:
        ctx.release(h)


def has_match():
    out, st = ctx.has_match(chars, "/abc/")
    drop([out])
    return st


def find(m):
    out, st = ctx.find(chars, nd[m])
    drop([out])
    return st


def find_starts(m):
    outs, st = ctx.find_starts(chars, nd[m], stats=True)
    drop(outs)
    return st


paths = {"has_match_abc": has_match}
for m in needles:
    paths["find_m%d" % m] = lambda m=m: find(m)
    paths["find_starts_m%d" % m] = lambda m=m: find_starts(m)
stats = {}
for _ in range(2):  # warm-up: every plan cached
    for name, f in paths.items():
        stats[name] = f()
want = F.plain_find(text, F.needle_masks("abc"))
out, _ = ctx.find(chars, nd[3])
assert ctx.decrypt_radix(ctx.download_radix(out)) == want[1] == 1
drop([out])
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
for n_ in nd.values():
    n_.close()
print(json.dumps(res), flush=True)
