#!/usr/bin/env python3
"""Point validation timing on one ctx: one JSON line with, per size (2^16, 2^18, 2^20), the median / min / max ms of
blocking device-resident checks -- G1 CURVE, G2 CURVE, G2 CURVE|SUBGROUP -- with the kernel time of the median call
(report.device_ms), the host twins at 16 threads on the same inputs (one run each), and the G2 table build
(msm_amd_g2_tables_build_device) the full G2 check would precede.
Usage: python tools/check_bench.py [--reps R] [--sizes 16,18,20] [--no-host] [--out FILE]"""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--no-host", action="store_true", help="skip the host twins")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import g2_ref as g
    from oracle import bn254_ref as o
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    res = {"metric": "check_points_ms", "reps": args.reps, "host_threads": 16, "subgroup_method": "a", "sizes": {}}

    def series(fn):
        fn()                                     # warm-up (allocations)
        ms, dev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            dev.append(rep["device_ms"])
            assert rep["n_invalid"] == 0
        mid = sorted(range(len(ms)), key=lambda i: ms[i])[len(ms) // 2]
        return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                "kernel_ms": round(dev[mid], 3)}

    def once(fn):
        t0 = time.perf_counter()
        rep, _ = fn()
        assert rep["n_invalid"] == 0
        return round((time.perf_counter() - t0) * 1e3, 1)

    try:
        for logn in (int(s) for s in args.sizes.split(",")):
            n = 1 << logn
            g1 = pkg.generate_instance_host(o.SEED_BASE, n)[0]
            g2 = pkg.g2_progression(g.encode_h2c(g.scalar_mul(3, g.GEN2)), g.encode_h2c(g.scalar_mul(5, g.GEN2)), n)
            d1, d2 = cfg.alloc(len(g1)), cfg.alloc(len(g2))
            cfg.to_device(d1, g1)
            cfg.to_device(d2, g2)
            entry = {"g1_curve_ms": series(lambda: cfg.check_points_device(d1, n, checks=pkg.CHECK_CURVE)),
                     "g2_curve_ms": series(lambda: cfg.g2_check_points_device(d2, n, checks=pkg.CHECK_CURVE)),
                     "g2_full_ms": series(lambda: cfg.g2_check_points_device(d2, n, checks=3))}
            t0 = time.perf_counter()
            tables = cfg.g2_tables_build_device(d2, n)
            entry["g2_tables_build_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            cfg.g2_tables_free(tables)
            entry["g2_full_over_tables_build"] = round(entry["g2_full_ms"]["median"] / entry["g2_tables_build_ms"], 3)
            cfg.free(d1)
            cfg.free(d2)
            if not args.no_host:
                entry["host_g1_curve_ms"] = once(lambda: pkg.host_check_points(g1, n, checks=1, threads=16, reasons=False))
                entry["host_g2_curve_ms"] = once(lambda: pkg.host_g2_check_points(g2, n, checks=1, threads=16, reasons=False))
                entry["host_g2_full_ms"] = once(lambda: pkg.host_g2_check_points(g2, n, checks=3, threads=16, reasons=False))
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
