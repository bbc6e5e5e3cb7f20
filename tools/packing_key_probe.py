"""Packing-key load and export time on the device: the full blob (fr_load_packing_key: one
201 / 151 MB upload, then the byte limbs) against the compact blob
(fr_load_packing_key_compact: the 63 / 31 MB of planes uploaded, masks and bodies rebuilt by
one kernel, then the byte limbs).  One process per FFT point; after one warm-up of each, 5
calls of each alternate.  Every call returns synchronised, so a host clock around the call is
its time.  The compact load's stages come from HIP events of further loads under
fr_set_profiling, in a pass of their own.  The two exports are timed the same way.  One JSON
object per point.
Usage: python3 tools/packing_key_probe.py [--point k1n2048|k2n1024] [--reps 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = {"k1n2048": (1, 2048), "k2n1024": (2, 1024)}


def probe(point: str, reps: int) -> dict:
    sys.path.insert(0, os.path.join(REPO, "fhe-regex_amd"))
    import fheregex as F

    k, N = POINTS[point]
    p = F.default_params(k=k, N=N)
    with open(os.path.join(REPO, "tests", "golden", "client_key"), "rb") as f:
        client_key = f.read()
    client = F.Context(device=-1, params=p)
    client.load_client_key(client_key)
    client.gen_packing_key(bytes(range(32)), compact=True)
    full = client.export_packing_key()
    blob = client.export_packing_key_compact()
    server = F.Context(device=0, params=p)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def stats(t):
        return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}

    load_full = lambda: server.load_packing_key(full)
    load_compact = lambda: server.load_packing_key_compact(blob)
    timed(load_full)
    timed(load_compact)
    t_full, t_compact = [], []
    for _ in range(reps):
        t_full.append(timed(load_full))
        t_compact.append(timed(load_compact))
    # exports, from the compact install (both forms are available)
    server.export_packing_key()
    server.export_packing_key_compact()
    x_full, x_compact = [], []
    for _ in range(reps):
        x_full.append(timed(server.export_packing_key))
        x_compact.append(timed(server.export_packing_key_compact))
    same = bool((server.export_packing_key() == full).all() and (server.export_packing_key_compact() == blob).all())
    # the stages, by HIP events, in a pass of their own
    server.set_profiling(1)
    split = []
    for _ in range(reps):
        load_compact()
        split.append(server.packing_key_load_timers())
    stages = {name: stats([s[i] for s in split]) for i, name in enumerate(("h2d", "expand", "limbs"))}

    return {"point": point, "device": server.info(), "reps": reps, "full_bytes": len(full), "compact_bytes": len(blob),
            "full_load": stats(t_full), "compact_load": stats(t_compact), "compact_split": stages,
            "full_export": stats(x_full), "compact_export": stats(x_compact), "device_key_equals_host": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=sorted(POINTS))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.point:
        print(json.dumps(probe(a.point, a.reps)), flush=True)
        return
    for point in POINTS:  # a fresh process per point
        subprocess.run([sys.executable, os.path.abspath(__file__), "--point", point, "--reps", str(a.reps)], check=True)


if __name__ == "__main__":
    main()
