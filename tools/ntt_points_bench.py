#!/usr/bin/env python3
"""Time the transform over G1 points on one GPU against its building block and its host twin.

INVERSE (the monomial SRS to the Lagrange SRS), MSM_AMD_NTT_ROOT_H2C, device-resident MSM_AMD_POINT_PREPARED records in and
out, n = 2^12, 2^16, 2^20 generated points.  Per size, after an untimed load that ramps the clock and --warmup calls, the
medians of --iters calls (fewer at 2^20, see ITERS): kernel_ms as the call reports it and the wall time of the blocking
call.  Same run, same build, the yardstick: msm_amd_mul_points_device(MSM_AMD_MUL_BASE_EACH) -- the ladder the butterflies
run -- on n/2 prepared records with random scalars, times the number of laddered levels (log_n - 1), plus one such call on n
records for the n^-1 pass; wall time of the blocking call, which is what that call can report.  ratio = call time of the
transform over the yardstick; the gate is 1.25.
Time per level: the kernel times come from a kernel trace, in a run of its own (the profiler slows the host, so no call
time is taken from it).  Levels with at least 64 blocks (l <= log_n - 6) share one factor per wave, levels 2 .. log_n all
walk a ladder:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ntt_points_bench.py --one-call 20
  python tools/ntt_points_bench.py --one-call 20 --from-trace DIR/.../*_kernel_trace.csv [--levels-out profiles/ntt_points_levels.txt]
The host twin runs at 16 threads on the same box up to --host-log (its bytes must equal the device's).
Writes profiles/ntt_points_bench.json.

  python tools/ntt_points_bench.py [--logs 12 16 20] [--host-log 16] [--out profiles/ntt_points_bench.json]
"""
import argparse
import importlib
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mle_bench import median_ms  # noqa: E402
from ntt_bench import commit, shader_clock_mhz  # noqa: E402

GATE = 1.25
ITERS = {12: 20, 16: 10, 20: 5}          # a call at 2^20 is ten million ladders


def wall_ms(call, warmup, iters):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def one_call(pkg, log_n):
    """three INVERSE calls at 2^log_n, prepared in and out: what runs under the kernel trace"""
    n = 1 << log_n
    cfg = pkg.setup_metal_state(0)
    try:
        d_aff, _ = cfg.generate_instance(1234 + log_n, n, True)
        d_in, d_out = cfg.bases_prepare_device(d_aff, n, pkg.POINT_H2C_AFFINE), cfg.alloc(64 * n)
        dom = cfg.ntt_domain(pkg.NTT_ROOT_H2C, log_n)
        for _ in range(3):
            print("kernel_ms", cfg.ntt_points_device(dom, d_in, d_out, pkg.NTT_INVERSE, pkg.POINT_PREPARED, pkg.POINT_PREPARED),
                  flush=True)
    finally:
        cfg.close()


def from_trace(path, log_n, out):
    """the kernels of the LAST transform in a rocprofv3 kernel trace, summed per level"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "nttp_" in r["Kernel_Name"] or "mul_normalise" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    call = rows[[i for i, r in enumerate(rows) if "nttp_load" in r["Kernel_Name"]][-1]:]
    ms = lambda rs: sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs) / 1e6   # noqa: E731
    named = lambda stem: [r for r in call if stem in r["Kernel_Name"]]   # noqa: E731
    lv, nm = named("nttp_level"), named("nttp_normalise")
    if not lv or len(lv) % log_n:
        raise SystemExit(f"ntt_points_bench.py: {len(lv)} level launches are not those of a transform of 2^{log_n} points")
    per = len(lv) // log_n
    lines = ["# tools/ntt_points_bench.py --from-trace: kernel time per level of one INVERSE transform at 2^%d, %d launches per "
             "level (rocprofv3 --kernel-trace)" % (log_n, per), "# level  blocks  wave_uniform  butterflies_ms  normalise_ms"]
    for l in range(1, log_n + 1):
        part = slice((l - 1) * per, l * per)
        lines.append("%-7d %-7d %-13s %-15.3f %.3f" % (l, (1 << log_n) >> l, ((1 << log_n) >> l) >= 64, ms(lv[part]), ms(nm[part])))
    lines.append("# load %.3f ms, n^-1 ladder %.3f ms, last normalise %.3f ms, first start to last end %.3f ms" % (
        ms(call[:1]), ms(named("nttp_scale")), ms(named("mul_normalise")),
        (int(call[-1]["End_Timestamp"]) - int(call[0]["Start_Timestamp"])) / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one-call", type=int, default=None, metavar="LOG_N", help="only run the call three times (for a trace)")
    ap.add_argument("--from-trace", default=None, metavar="CSV", help="only sum a kernel trace per level")
    ap.add_argument("--levels-out", default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-log", type=int, default=16, help="the host twin runs up to this size")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_points_bench.json"))
    args = ap.parse_args()
    if args.from_trace:
        return from_trace(args.from_trace, args.one_call or 20, args.levels_out)
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    if args.one_call is not None:
        return one_call(pkg, args.one_call)
    cfg = pkg.setup_metal_state(0)
    prepared, inverse = pkg.POINT_PREPARED, pkg.NTT_INVERSE
    rows = []
    try:
        for log_n in args.logs:
            n = 1 << log_n
            iters = ITERS.get(log_n, 5)
            d_aff, d_sc = cfg.generate_instance(1234 + log_n, n, True)
            d_in = cfg.bases_prepare_device(d_aff, n, pkg.POINT_H2C_AFFINE)
            d_out = cfg.alloc(64 * n)
            dom = cfg.ntt_domain(pkg.NTT_ROOT_H2C, log_n)
            call = lambda: cfg.ntt_points_device(dom, d_in, d_out, inverse, prepared, prepared)   # noqa: E731
            half = lambda: cfg.mul_points_device(d_sc, d_in, n // 2, d_out, pkg.MUL_BASE_EACH, pkg.SCALAR_MONT_LE,   # noqa: E731
                                                 prepared, prepared)
            full = lambda: cfg.mul_points_device(d_sc, d_in, n, d_out, pkg.MUL_BASE_EACH, pkg.SCALAR_MONT_LE,   # noqa: E731
                                                 prepared, prepared)
            if not rows:
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    half()
            h_ms, h_min, h_max = wall_ms(half, args.warmup, iters)
            f_ms, f_min, f_max = wall_ms(full, args.warmup, iters)
            k_ms, w_ms = median_ms(call, args.warmup, iters)
            clk = shader_clock_mhz(cfg.device())
            yard = (log_n - 1) * h_ms + f_ms
            row = {"log_n": log_n, "iters": iters, "kernel_ms": round(k_ms, 3), "call_ms": round(w_ms, 3), "sclk_mhz": clk,
                   "mul_each_half_ms": round(h_ms, 3), "mul_each_half_min_max_ms": [round(h_min, 3), round(h_max, 3)],
                   "mul_each_full_ms": round(f_ms, 3), "mul_each_full_min_max_ms": [round(f_min, 3), round(f_max, 3)],
                   "laddered_levels": log_n - 1, "yardstick_ms": round(yard, 3), "ratio": round(w_ms / yard, 3),
                   "ratio_bound": GATE, "within_bound": bool(w_ms / yard <= GATE),
                   "ladders": (log_n - 1) * (n // 2) - (n // 2 - 1) + n,      # lanes with i = 0 walk none; n for n^-1
                   "host_twin_16_threads_ms": None, "speedup_over_host": None}
            if log_n <= args.host_log:
                aff = cfg.to_host(d_aff, 64 * n)                      # the twin takes the host layout
                t0 = time.perf_counter()
                ref = pkg.host_ntt_points(aff, pkg.NTT_ROOT_H2C, log_n, inverse, pkg.POINT_H2C_AFFINE, pkg.POINT_H2C_AFFINE,
                                          threads=16)
                row["host_twin_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                row["speedup_over_host"] = round(row["host_twin_16_threads_ms"] / w_ms, 1)
                d_chk = cfg.alloc(64 * n)
                cfg.ntt_points_device(dom, d_in, d_chk, inverse, prepared, pkg.POINT_H2C_AFFINE)
                same = cfg.to_host(d_chk, 64 * n) == ref
                cfg.free(d_chk)
                if not same:
                    raise SystemExit(f"ntt_points_bench.py: GPU and host twin differ at log_n={log_n}")
            rows.append(row)
            print(json.dumps(row), flush=True)
            dom.free()
            for p in (d_aff, d_sc, d_in, d_out):
                cfg.free(p)
    finally:
        cfg.close()
    result = {
        "tool": "tools/ntt_points_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "warmup": args.warmup, "prewarm_ms": args.prewarm_ms,
        "mul_chunk": int(os.environ.get("MSM_AMD_MUL_CHUNK", "-1")),
        "setting": "INVERSE, ROOT_H2C, device-resident PREPARED records in and out, out of place; medians of the timed calls; "
                   "yardstick = (log_n - 1) x mul_points_device(BASE_EACH, n/2) + mul_points_device(BASE_EACH, n), wall time",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
