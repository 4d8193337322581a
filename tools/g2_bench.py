#!/usr/bin/env python3
"""G2 MSM timing on one ctx: one JSON line with, per size (2^16, 2^18, 2^20), the median ms of a lone blocking G2 call
on device-resident inputs, the G1 lone call on device-resident inputs of the same size, their ratio and the G2 stage
split from the library's HIP events (msm_amd_last_timings: G1's definitions -- `accumulate` is the accumulate kernel
alone, the combine pass counts under `combine_reduce_copy`, `gpu_total` is the sum of the spans), plus the CPU G2 MSM
at 2^16.
Next to that per-call figure (`g2_ms`, the caller layout converted on every call), the same scalars through prepared
bases (`prepared_ms`) and through precomputed window tables at the automatic window (`tables_ms`): median, min and max
of each series, their stage splits, the table's window / windows / bytes and `tables_build_ms`; and one host-caller row
at 2^20: msm_g2 (host points and scalars) against msm_g2_prepared and msm_g2_tables (host scalars only).
Usage: python tools/g2_bench.py [--reps R] [--sizes 16,18,20] [--sweep 14,16,18] [--out FILE]"""
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
    ap.add_argument("--sweep", default="", help="table windows to time besides the automatic one, e.g. 14,16,18")
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
            def series(d_points, layout):
                """lone blocking msm_g2_device calls: (ms per rep, stage split per rep)"""
                ms, split = [], []
                cfg.msm_g2_device(ds, d_points, n, scalar_layout=1, point_layout=layout)   # warm-up (allocations)
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    cfg.msm_g2_device(ds, d_points, n, scalar_layout=1, point_layout=layout)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    t = cfg.timings()
                    split.append({"convert": t.convert_ms, "digits": t.digits_ms, "sort": t.sort_ms,
                                  "accumulate": t.accumulate_ms, "combine_reduce_copy": t.reduce_ms,
                                  "host_horner": t.final_ms, "gpu_total": t.total_gpu_ms, "window": t.window_size})
                return ms, split

            def summary(ms, split):
                mid = sorted(range(len(ms)), key=lambda i: ms[i])[len(ms) // 2]
                return (round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3),
                        {k: (round(v, 3) if isinstance(v, float) else v) for k, v in split[mid].items()})

            g2, split = series(dp, pkg.G2_POINT_H2C_AFFINE)
            d_prep = cfg.g2_bases_prepare_device(dp, n)
            prep, prep_split = series(d_prep, pkg.G2_POINT_PREPARED)
            t0 = time.perf_counter()
            tables = cfg.g2_tables_build_device(dp, n)
            tables_build_ms = (time.perf_counter() - t0) * 1e3
            info = cfg.g2_tables_info(tables)
            tab, tab_split = series(tables, pkg.G2_POINT_TABLES)
            sweep = {}
            for c in (int(x) for x in args.sweep.split(",") if x):
                if (254 // c + 1) * n >= 1 << 31:
                    continue
                tc = cfg.g2_tables_build_device(dp, n, window_size=c)
                ms, _ = series(tc, pkg.G2_POINT_TABLES)
                cfg.g2_tables_free(tc)
                sweep[str(c)] = round(statistics.median(ms), 3)
            host_row = None
            if logn == 20:   # a host caller: points and scalars in host memory against scalars only
                def host_series(fn):
                    fn()
                    ms = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        fn()
                        ms.append((time.perf_counter() - t0) * 1e3)
                    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
                host_row = {"msm_g2_ms": host_series(lambda: cfg.msm_g2(sc, pts, n, scalar_layout=1)),
                            "msm_g2_prepared_ms": host_series(lambda: cfg.msm_g2_prepared(sc, d_prep, n, scalar_layout=1)),
                            "msm_g2_tables_ms": host_series(lambda: cfg.msm_g2_tables(sc, tables, scalar_layout=1))}
            cfg.g2_tables_free(tables)
            cfg.free(d_prep)
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
            g2_med, g2_min, g2_max, g2_split = summary(g2, split)
            entry = {"g2_ms": g2_med, "g1_ms": round(statistics.median(g1), 3), "split_ms": g2_split}
            entry["g2_over_g1"] = round(entry["g2_ms"] / entry["g1_ms"], 2)
            entry["g2_min_ms"], entry["g2_max_ms"] = g2_min, g2_max
            (entry["prepared_ms"], entry["prepared_min_ms"], entry["prepared_max_ms"],
             entry["prepared_split_ms"]) = summary(prep, prep_split)
            (entry["tables_ms"], entry["tables_min_ms"], entry["tables_max_ms"],
             entry["tables_split_ms"]) = summary(tab, tab_split)
            entry["tables_window"], entry["tables_windows"] = info["window_size"], info["num_windows"]
            entry["tables_bytes"] = info["device_bytes"]
            entry["tables_build_ms"] = round(tables_build_ms, 1)
            entry["tables_over_g2"] = round(entry["tables_ms"] / entry["g2_ms"], 3)
            entry["prepared_over_g2"] = round(entry["prepared_ms"] / entry["g2_ms"], 3)
            if sweep:
                entry["tables_sweep_ms"] = sweep
            if host_row:
                res["host_caller_2^20"] = host_row
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
