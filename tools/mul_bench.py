#!/usr/bin/env python3
"""Batch scalar multiplication timing on one ctx: one JSON line with, per size (2^16, 2^18, 2^20), group (G1, G2) and
base mode (BASE_ONE, BASE_EACH on the replicated base), the median / min / max ms of blocking device-resident calls --
output as halo2curves affine records and as *_PREPARED records -- and the host twins at 16 threads on the same inputs
(one run each).  A blocking call is the device time plus one stream wait: there is no per-kernel event in these calls.
Usage: python tools/mul_bench.py [--reps R] [--sizes 16,18,20] [--no-host] [--out FILE]"""
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
    ap.add_argument("--no-host", action="store_true", help="skip the host twins")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import g2_ref as g
    from oracle import bn254_ref as o
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    res = {"metric": "mul_points_ms", "reps": args.reps, "host_threads": 16, "plan": pkg.mul_plan(1), "sizes": {}}

    def series(fn):
        fn()                                     # warm-up (allocations)
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

    def once(fn):
        t0 = time.perf_counter()
        fn()
        return round((time.perf_counter() - t0) * 1e3, 1)

    base = {1: o.encode_affine_h2c(o.scalar_mul(12345, o.GEN)), 2: g.encode_h2c(g.scalar_mul(12345, g.GEN2))}
    try:
        for logn in (int(s) for s in args.sizes.split(",")):
            n = 1 << logn
            scalars = pkg.generate_instance_host(o.SEED_BASE, n)[1]
            d_sc = cfg.alloc(len(scalars))
            cfg.to_device(d_sc, scalars)
            entry = {}
            for group in (1, 2):
                g2 = group == 2
                prepared = pkg.G2_POINT_PREPARED if g2 else pkg.POINT_PREPARED
                size = len(base[group])
                d_one, d_each, d_out = cfg.alloc(size), cfg.alloc(n * size), cfg.alloc(n * size)
                cfg.to_device(d_one, base[group])
                cfg.to_device(d_each, base[group] * n)
                e = {}
                for mode, name, d_pts in ((pkg.MUL_BASE_ONE, "one", d_one), (pkg.MUL_BASE_EACH, "each", d_each)):
                    for lo, lname in ((0, "affine"), (prepared, "prepared")):
                        e[f"{name}_to_{lname}_ms"] = series(
                            lambda: cfg.mul_points_device(d_sc, d_pts, n, d_out, mode, 0, 0, lo, g2=g2))
                    if not args.no_host:
                        pts = base[group] * (n if mode == pkg.MUL_BASE_EACH else 1)
                        e[f"host_{name}_ms"] = once(
                            lambda: pkg.host_mul_points(scalars, pts, n, mode, g2=g2, threads=16))
                for p in (d_one, d_each, d_out):
                    cfg.free(p)
                entry["g2" if g2 else "g1"] = e
                print(f"2^{logn} {'g2' if g2 else 'g1'}: {json.dumps(e)}", file=sys.stderr, flush=True)
            cfg.free(d_sc)
            res["sizes"][f"2^{logn}"] = entry
    finally:
        cfg.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
