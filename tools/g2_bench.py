#!/usr/bin/env python3
"""G2 MSM timing on one ctx: one JSON line with, per size (2^16, 2^18, 2^20), the median ms of a lone blocking G2 call
on device-resident inputs, the G1 lone call on device-resident inputs of the same size, their ratio and the G2 stage
split from the library's HIP events (msm_amd_last_timings), plus the CPU G2 MSM at 2^16.
Usage: python tools/g2_bench.py [--reps R] [--sizes 16,18,20] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import g2_ref as g
    from oracle import bn254_ref as o
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    res = {"metric": "g2_msm_lone_ms", "reps": args.reps, "sizes": {}}
    try:
        for logn in (int(s) for s in args.sizes.split(",")):
            n = 1 << logn
            pts = pkg.g2_progression(g.encode_h2c(g.scalar_mul(3, g.GEN2)), g.encode_h2c(g.scalar_mul(5, g.GEN2)), n)
            w = np.random.default_rng(logn).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x0FFFFFFF
            sc = w.tobytes()
            ds, dp = cfg.alloc(len(sc)), cfg.alloc(len(pts))
            cfg.to_device(ds, sc)
            cfg.to_device(dp, pts)
            g2, split = [], []
            cfg.msm_g2_device(ds, dp, n, scalar_layout=1)   # warm-up (allocations)
            for _ in range(args.reps):
                t0 = time.perf_counter()
                cfg.msm_g2_device(ds, dp, n, scalar_layout=1)
                g2.append((time.perf_counter() - t0) * 1e3)
                t = cfg.timings()
                split.append({"convert": t.convert_ms, "digits": t.digits_ms, "sort": t.sort_ms,
                              "accumulate_combine": t.accumulate_ms, "reduce_copy": t.reduce_ms,
                              "host_horner": t.final_ms, "gpu_total": t.total_gpu_ms, "window": t.window_size})
            cfg.free(ds)
            cfg.free(dp)
            gp, gs = cfg.generate_instance(o.SEED_BASE, n, True)
            g1 = []
            cfg.msm_batch_device([gs], [gp], [n])
            for _ in range(args.reps):
                t0 = time.perf_counter()
                cfg.msm_batch_device([gs], [gp], [n])
                g1.append((time.perf_counter() - t0) * 1e3)
            cfg.free(gp)
            cfg.free(gs)
            mid = sorted(range(len(g2)), key=lambda i: g2[i])[len(g2) // 2]
            entry = {"g2_ms": round(statistics.median(g2), 3), "g1_ms": round(statistics.median(g1), 3),
                     "split_ms": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in split[mid].items()}}
            entry["g2_over_g1"] = round(entry["g2_ms"] / entry["g1_ms"], 2)
            res["sizes"][f"2^{logn}"] = entry
            if logn == 16:
                t0 = time.perf_counter()
                pkg.host_msm_g2(sc, pts, n, threads=0, scalar_layout=1)
                res["host_g2_2^16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    finally:
        cfg.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
