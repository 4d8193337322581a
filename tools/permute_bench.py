#!/usr/bin/env python3
"""Time halo2's permuted lookup columns on one GPU.

msm_amd_fr_lookup_permute with both outputs, MSM_AMD_SCALAR_MONT_LE, n = n_rows = 2^16 .. 2^22 on four input columns:
uniform draws over the rows, a column that is half one row (row 0), a column that is all one row, and a shuffle of the
table.  The call takes host buffers, so its wall time (median of --iters blocking calls after --warmup more, the clock
pre-warmed) holds the upload of the column and the download of A' and S'; beside it the host twin at 16 threads on the same
box, whose bytes must equal the device's, and the bytes the kernels must move (the column in, one table row per position,
A' and S' out: 128 bytes per position) against 8 TB/s.
Kernel time: from a kernel trace, in a run of its own per setting (the profiler slows the host, so no call time is taken
from it); the kernels of the last of K calls per case, summed per phase (count: the probe; scan: the reductions and scans
with the compaction; owner: the maximum scan of MSM_AMD_PERMUTE_FILL=scan; fill).  The memsets of a call (fill kernels of the
runtime in the trace) are not in these sums.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/permute_bench.py --trace-calls 3
  python tools/permute_bench.py --trace-calls 3 --from-trace DIR/.../*_kernel_trace.csv --key phases_ms
The same with MSM_AMD_PERMUTE_FILL=scan in the environment of the traced run and --key phases_scan_ms gives the A/B of the
fill (--ab-out writes it as a text table, profiles/permute_ab.txt), and with MSM_AMD_PERMUTE_TILE_LOG=T, --logs 22 --dists
uniform and --key phases_tile_log_T the tile sweep.  Writes profiles/permute_bench.json.

  python tools/permute_bench.py [--logs 16 18 20 22] [--iters 10] [--warmup 2] [--out profiles/permute_bench.json]
"""
import argparse
import ctypes
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

DISTRIBUTIONS = ("uniform", "half_one_row", "all_one_row", "shuffle")
MUST_MOVE = 32 * 4
PHASES = (("count", "fr_lookup_probe_kernel"), ("scan", "fr_permute_reduce_kernel"), ("scan", "fr_permute_scan_kernel"),
          ("owner", "fr_permute_max_"), ("fill", "fr_permute_fill_kernel"))


def table_rows(rng, n):
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x1F                                               # every record < 2^253 < r
    return raw


def draw(rng, rows, n, dist):
    if dist == "all_one_row":
        idx = np.zeros(n, dtype=np.int64)
    elif dist == "shuffle":
        idx = rng.permutation(n)
    else:
        idx = rng.integers(0, len(rows), size=n)
        if dist == "half_one_row":
            idx[::2] = 0
    return rows[idx].tobytes()


def cases(logs, dists):
    """(log_n, distribution) in the order every mode runs them"""
    return [(log_n, dist) for log_n in logs for dist in dists]


def from_trace(path, todo, calls, key, out):
    """the kernels of the LAST call of every case in a rocprofv3 kernel trace, summed per phase, into row[key] of `out`"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if any(stem in r["Kernel_Name"] for _, stem in PHASES)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "fr_permute_fill_kernel" in r["Kernel_Name"]]
    if len(ends) != calls * len(todo):
        raise SystemExit(f"permute_bench.py: {len(ends)} fill launches in the trace, expected {calls * len(todo)}")
    with open(out) as f:
        result = json.load(f)
    for k, (log_n, dist) in enumerate(todo):
        last = k * calls + calls - 1
        part = rows[ends[last - 1] + 1 if last else 0:ends[last] + 1]
        phases = {}
        for name, stem in PHASES:
            ms = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in part if stem in r["Kernel_Name"]) / 1e6
            phases[name] = round(phases.get(name, 0) + ms, 4)
        phases["kernels_ms"] = round(sum(phases.values()), 4)
        phases["first_start_to_last_end_ms"] = round((int(part[-1]["End_Timestamp"]) - int(part[0]["Start_Timestamp"])) / 1e6, 4)
        phases["launches"] = len(part)
        for row in result["rows"]:
            if row["log_n"] == log_n and row["distribution"] == dist:
                row[key] = phases
        print(json.dumps({"log_n": log_n, "distribution": dist, key: phases}), flush=True)
    result.setdefault("phases_source", "rocprofv3 --kernel-trace of --trace-calls K, the last call of every case, one run per key")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def write_ab(out, ab_out):
    with open(out) as f:
        result = json.load(f)
    lines = ["# tools/permute_bench.py: msm_amd_fr_lookup_permute, n = n_rows, both outputs: kernel time of one call (rocprofv3",
             "# --kernel-trace, the last of three calls per case, one traced run per form on %s; the memsets of a call not included)," % result["box"],
             "# MSM_AMD_PERMUTE_FILL=search (binary search for the owner) against =scan (heads scattered, maximum scan)",
             "# log_n  column         search: count scan fill = sum        scan: count scan owner fill = sum          scan / search"]
    for r in result["rows"]:
        a, b = r.get("phases_ms"), r.get("phases_scan_ms")
        if not a or not b:
            continue
        lines.append("%-7d %-14s %.4f %.4f %.4f = %.4f        %.4f %.4f %.4f %.4f = %.4f        %.3f" % (
            r["log_n"], r["distribution"], a["count"], a["scan"], a["fill"], a["kernels_ms"],
            b["count"], b["scan"], b["owner"], b["fill"], b["kernels_ms"], b["kernels_ms"] / a["kernels_ms"]))
    with open(ab_out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prewarm-ms", type=int, default=1500)
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 18, 20, 22])
    ap.add_argument("--dists", nargs="*", default=list(DISTRIBUTIONS), choices=DISTRIBUTIONS)
    ap.add_argument("--trace-calls", type=int, default=None, metavar="K", help="only run every case K times (for a trace)")
    ap.add_argument("--from-trace", default=None, metavar="CSV", help="only sum a kernel trace per phase into --out")
    ap.add_argument("--key", default="phases_ms", help="where --from-trace puts the sums in a row")
    ap.add_argument("--ab-out", default=None, help="only write the A/B of the fill from --out as a text table")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permute_bench.json"))
    args = ap.parse_args()
    todo = cases(args.logs, args.dists)
    if args.from_trace:
        return from_trace(args.from_trace, todo, args.trace_calls or 3, args.key, args.out)
    if args.ab_out:
        return write_ab(args.out, args.ab_out)
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    out_rows, clocks = [], []
    try:
        if not args.trace_calls:
            big = 1 << max(args.logs)
            d_x = cfg.alloc(32 * big)
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                cfg.fr_shift_device(d_x, big, d_x, bytes(32))
            cfg.free(d_x)
        for log_n, dist in todo:
            n = 1 << log_n
            rng = np.random.default_rng(1000 * log_n + DISTRIBUTIONS.index(dist))
            rows = table_rows(np.random.default_rng(log_n), n)
            data = draw(rng, rows, n, dist)
            a, s = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
            h = cfg.fr_lookup_build(rows.tobytes())
            try:
                def call():
                    t0 = time.perf_counter()
                    report = cfg.fr_lookup_permute(h, data, a_out=a, s_out=s)[2]
                    return (time.perf_counter() - t0) * 1e3, report
                if args.trace_calls:
                    for _ in range(args.trace_calls):
                        call()
                    continue
                for _ in range(args.warmup):
                    call()
                walls = [call() for _ in range(args.iters)]
                wall, report = statistics.median(w for w, _ in walls), walls[-1][1]
                clk = shader_clock_mhz(cfg.device())
                clocks.append(clk)
                row = {"log_n": log_n, "distribution": dist, "wall_ms": round(wall, 4), "must_move_bytes": MUST_MOVE * n,
                       "hbm_bound_ms": round(MUST_MOVE * n / HBM_BYTES_PER_S * 1e3, 4), "sclk_mhz": clk, **report,
                       "plan": pkg.test_fr_permute_plan(n)}
                t0 = time.perf_counter()
                twin = pkg.host_fr_lookup_permute(rows.tobytes(), data, threads=16)
                row["host_twin_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                row["speedup_over_host"] = round(row["host_twin_16_threads_ms"] / wall, 1)
                if (a.raw, s.raw) != twin[:2]:
                    raise SystemExit(f"permute_bench.py: GPU and host twin differ: {dist} at 2^{log_n}")
                out_rows.append(row)
                print(json.dumps(row), flush=True)
            finally:
                h.free()
    finally:
        cfg.close()
    if args.trace_calls:
        return
    result = {
        "tool": "tools/permute_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(), "sclk_mhz": clocks,
        "iters": args.iters, "warmup": args.warmup, "prewarm_ms": args.prewarm_ms, "must_move_bytes_per_position": MUST_MOVE,
        "setting": "host buffers, MONT_LE, n = n_rows, both outputs; wall time of the blocking call, median; there is no target",
        "rows": out_rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
