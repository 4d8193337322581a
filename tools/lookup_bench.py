#!/usr/bin/env python3
"""Time the lookup calls on one GPU.

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE; the clock is pre-warmed the way bench.py does it; every figure is the
median of --iters timed calls after --warmup more, kernel_ms as the call reports it.  Everything that is compared runs
in this one command:
  build        msm_amd_fr_lookup_build_device at 2^16 and 2^20 rows
  lookup       msm_amd_fr_lookup_multiplicities_device at 2^20 and 2^24 lookups into each table, on three distributions
               (uniform over the rows, half zeros -- the value of row 0 --, all equal), with the three counting forms
               (MSM_AMD_LOOKUP_COUNT = block / wave / lane) alternated --alternations times; bytes moved per lookup counted from
               the shapes (32 in, 4 idx out, one slot and one row read per probe step ~ 36, 4 for the counter) against 8 TB/s
  twin         the host twin at 16 threads at 2^20 lookups, per distribution
  atomics      the integer-atomic rate: lookups per second of the lane form on the all-equal column (every add on one
               dword) and on the uniform column (one dword in each of 64 rows)
  prefix_sum   next to prefix_product at 2^24, alternated; shift next to fr_map(ADD) at 2^24, alternated
Writes profiles/lookup_bench.json.

  python tools/lookup_bench.py [--iters 20] [--warmup 3] [--out profiles/lookup_bench.json]
"""
import argparse
import importlib
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ntt_bench import HBM_BYTES_PER_S, commit, shader_clock_mhz  # noqa: E402

DISTRIBUTIONS = ("uniform", "half_zeros", "all_equal")
BYTES_PER_LOOKUP = 32 + 4 + 36 + 4


def records(rng, n):
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1F                                               # every record < 2^253 < r
    return raw


def draw(rng, rows, n, dist):
    if dist == "all_equal":
        idx = np.zeros(n, dtype=np.int64)
    else:
        idx = rng.integers(0, len(rows), size=n)
        if dist == "half_zeros":
            idx[::2] = 0
    return rows[idx].tobytes()


def median_ms(call, iters, warmup):
    for _ in range(warmup):
        call()
    return statistics.median(call() for _ in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500)
    ap.add_argument("--row-logs", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--lookup-logs", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--vector-log", type=int, default=24)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    rng = np.random.default_rng(11)
    rows_out, builds, vectors, clocks = [], [], [], []
    try:
        # ---- vectors: prefix_sum next to prefix_product, shift next to ADD ------------------------------------------
        n = 1 << args.vector_log
        a = records(rng, n).tobytes()
        d_a, d_b, d_out = cfg.alloc(32 * n), cfg.alloc(32 * n), cfg.alloc(32 * n)
        cfg.to_device(d_a, a)
        cfg.to_device(d_b, a)
        k = (12345).to_bytes(32, "little")
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
            cfg.fr_map_device(pkg.FR_MUL, d_a, d_b, None, n, d_out)
        calls = {
            "prefix_product": lambda: cfg.fr_prefix_product_device(d_a, n, d_out),
            "prefix_sum": lambda: cfg.fr_prefix_sum_device(d_a, n, d_out),
            "add": lambda: cfg.fr_map_device(pkg.FR_ADD, d_a, d_b, None, n, d_out),
            "shift": lambda: cfg.fr_shift_device(d_a, n, d_out, k),
        }
        for rnd in range(args.alternations):
            for name, call in calls.items():
                vectors.append({"op": name, "log_n": args.vector_log, "round": rnd,
                                "kernel_ms": round(median_ms(call, args.iters, args.warmup), 4)})
                print(json.dumps(vectors[-1]), flush=True)
        add_ms = statistics.median(v["kernel_ms"] for v in vectors if v["op"] == "add")
        for d in (d_a, d_b, d_out):
            cfg.free(d)
        # ---- tables ----------------------------------------------------------------------------------------------
        for row_log in args.row_logs:
            n_rows = 1 << row_log
            rows = records(rng, n_rows)
            d_t = cfg.alloc(32 * n_rows)
            cfg.to_device(d_t, rows.tobytes())
            built = []

            def build():
                h = cfg.fr_lookup_build_device(d_t, n_rows)
                built.append(h)
                if len(built) > 1:
                    built.pop(0).free()
                return h.build_ms
            t0 = time.perf_counter()
            build_ms = median_ms(build, args.iters, args.warmup)
            wall_ms = (time.perf_counter() - t0) * 1e3 / (args.iters + args.warmup)
            h = built[0]
            info = h.info()
            builds.append({"row_log": row_log, "kernel_ms": round(build_ms, 4), "wall_ms_per_call": round(wall_ms, 4),
                           "rows_per_s": round(n_rows / build_ms * 1e3), **info})
            print(json.dumps(builds[-1]), flush=True)
            d_m = cfg.alloc(32 * n_rows)
            for lookup_log in args.lookup_logs:
                n = 1 << lookup_log
                d_in, d_idx = cfg.alloc(32 * n), cfg.alloc(4 * n)
                for dist in DISTRIBUTIONS:
                    data = draw(rng, rows, n, dist)
                    cfg.to_device(d_in, data)
                    forms = {"block": [], "wave": [], "lane": []}
                    for _ in range(args.alternations):
                        for form in forms:
                            os.environ["MSM_AMD_LOOKUP_COUNT"] = form
                            forms[form].append(median_ms(
                                lambda: cfg.fr_lookup_multiplicities_device(h, d_in, n, d_m, d_idx)[1], args.iters, args.warmup))
                    os.environ.pop("MSM_AMD_LOOKUP_COUNT")
                    clk = shader_clock_mhz(cfg.device())
                    clocks.append(clk)
                    row = {"row_log": row_log, "lookup_log": lookup_log, "distribution": dist, "sclk_mhz": clk}
                    for form, ms in forms.items():
                        row[form + "_ms"] = [round(x, 4) for x in ms]
                        row[form + "_lookups_per_s"] = round(n / statistics.median(ms) * 1e3)
                    shipped = statistics.median(forms["block"])
                    row["hbm_bound_ms"] = round(BYTES_PER_LOOKUP * n / HBM_BYTES_PER_S * 1e3, 4)
                    row["hbm_fraction"] = round(row["hbm_bound_ms"] / shipped, 3)
                    row["ratio_to_add_same_records"] = round(shipped / (add_ms * n / (1 << args.vector_log)), 2)
                    if lookup_log == 20:
                        t0 = time.perf_counter()
                        twin = pkg.host_fr_lookup_multiplicities(rows.tobytes(), data, threads=16, want_idx=False)
                        row["host_twin_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                        t0 = time.perf_counter()
                        cfg.fr_lookup_multiplicities_device(h, d_in, n, d_m, d_idx)
                        row["device_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
                        row["speedup_over_host"] = round(row["host_twin_16_threads_ms"] / row["device_wall_ms"], 1)
                        if cfg.to_host(d_m, 32 * n_rows) != twin[0]:
                            raise SystemExit(f"lookup_bench.py: GPU and host twin differ: {dist} at 2^{row_log} rows")
                    rows_out.append(row)
                    print(json.dumps(row), flush=True)
                cfg.free(d_in)
                cfg.free(d_idx)
            h.free()
            cfg.free(d_m)
            cfg.free(d_t)
    finally:
        cfg.close()
    result = {
        "tool": "tools/lookup_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "iters": args.iters, "warmup": args.warmup, "alternations": args.alternations,
        "prewarm_ms": args.prewarm_ms, "bytes_per_lookup": BYTES_PER_LOOKUP,
        "setting": "device-resident, MONT_LE; median of the timed calls; the counting forms alternated in one process",
        "vectors": vectors, "builds": builds, "lookups": rows_out,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
