"""Server-key load time on the device: the full arrays (fr_load_server_key: host Fourier
transform, one upload per lane geometry) against the compact blob (fr_load_server_key_compact:
bodies uploaded, masks expanded and the key transformed on the GPU).  One process per FFT
point; after one warm-up of each, 5 calls of each alternate.  Both calls return
synchronised, so a host clock around the call is the load time.  The compact path's stages
come from HIP events of one further load under fr_set_profiling.  One JSON object per point.
Usage: python3 tools/key_load_probe.py [--point k1n2048|k2n1024] [--reps 5]"""
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
    client.gen_server_key(bytes(range(32)), compact=True)
    ksk, bsk = client.export_server_key()
    blob = client.export_server_key_compact()
    server = F.Context(device=0, params=p)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    full = lambda: server.load_server_key(ksk, bsk)
    compact = lambda: server.load_server_key_compact(blob)
    timed(full)
    timed(compact)
    t_full, t_compact = [], []
    for _ in range(reps):
        t_full.append(timed(full))
        t_compact.append(timed(compact))
    server.set_profiling(1)
    timed(compact)
    split = dict(zip(("h2d_ms", "k_expand_ksk_ms", "k_expand_bsk_ms", "ksk_limbs_ms", "k_bsk_fourier_ms"),
                     (round(x, 4) for x in server.key_load_timers())))
    k2, b2 = server.export_server_key()
    same = bool((k2 == ksk).all() and (b2 == bsk).all())

    def stats(t):
        return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}

    return {"point": point, "device": server.info(), "reps": reps, "full_bytes": 8 * (len(ksk) + len(bsk)),
            "compact_bytes": len(blob), "full_load": stats(t_full), "compact_load": stats(t_compact),
            "compact_split": split, "device_key_equals_host": same}


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
