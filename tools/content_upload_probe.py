"""Content upload time on the device: the full LWE words (fr_upload_radix: one 16 KB copy per
block) against the compact blob (fr_upload_compact_str: the bodies and the slot list in one
copy, the masks expanded by k_expand_blocks).  One process per FFT point; for 16, 256 and
1,024 chars, after one warm-up of each, `reps` measurements of each alternate.  A
measurement is a host clock around the call plus a synchronising download of the last
character (fr_upload_radix returns synchronised, fr_upload_compact_str returns once
enqueued; the download makes both complete), and records the bytes handed to the call.  The
time until the call returns is kept too.  The expansion kernel's duration comes from HIP
events of further uploads under fr_set_profiling, in a pass of its own.  The handles are
released after every measurement, so every upload takes its slots from the free list.
One JSON object per point.
Usage: python3 tools/content_upload_probe.py [--point k1n2048|k2n1024] [--reps 7]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = {"k1n2048": (1, 2048), "k2n1024": (2, 1024)}
SIZES = (16, 256, 1024)


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def probe(point: str, reps: int) -> dict:
    sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
    import numpy as np

    import fheregex as F

    k, N = POINTS[point]
    p = F.default_params(k=k, N=N)
    with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
        client_key = f.read()
    client = F.Context(device=-1, params=p)
    client.load_client_key(client_key)
    server = F.Context(device=0, params=p)
    rng = np.random.default_rng(1)
    rows = []
    for n in SIZES:
        s = "".join(chr(c) for c in rng.integers(0x20, 0x7F, n))
        blob = client.encrypt_str_compact(s, bytes(range(32)))
        full = client.expand_compact_content(blob).reshape(n, 4, -1)

        def measure(upload, arg):
            t0 = time.perf_counter()
            hs = upload(arg)
            t1 = time.perf_counter()
            last = server.download_radix(hs[-1])
            t2 = time.perf_counter()
            ok = bool((last == full[-1]).all())
            for h in hs:
                server.release(h)
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, ok

        measure(server.upload_radix, full)
        measure(server.upload_compact_str, blob)
        t_full, t_compact, c_full, c_compact, ok = [], [], [], [], True
        for _ in range(reps):
            a = measure(server.upload_radix, full)
            b = measure(server.upload_compact_str, blob)
            t_full.append(a[0]), c_full.append(a[1]), t_compact.append(b[0]), c_compact.append(b[1])
            ok = ok and a[2] and b[2]
        rows.append({"chars": n, "full_bytes": [int(full.nbytes)] * reps, "compact_bytes": [len(blob)] * reps,
                     "full_upload": stats(t_full), "compact_upload": stats(t_compact),
                     "full_call_return": stats(c_full), "compact_call_return": stats(c_compact),
                     "last_char_equals_host": ok})
    # the kernel alone, by HIP events (a profiled upload waits for its kernel)
    server.set_profiling(1)
    for row, n in zip(rows, SIZES):
        blob = client.encrypt_str_compact("x" * n, bytes(range(32)))
        ms = []
        for _ in range(reps + 1):
            hs = server.upload_compact_str(blob)
            ms.append(server.content_expand_timer())
            for h in hs:
                server.release(h)
        row["k_expand_blocks"] = stats(ms[1:])
        row["expanded_bytes"] = 8 * 4 * n * (k * N + 1)
    return {"point": point, "device": server.info(), "reps": reps, "sizes": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=sorted(POINTS))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.point:
        print(json.dumps(probe(a.point, a.reps)), flush=True)
        return
    for point in POINTS:  # a fresh process per point
        subprocess.run([sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(a.reps)], check=True)


if __name__ == "__main__":
    main()
