#!/usr/bin/env python3
"""Time the sparse product over Fr on one GPU against its host twin.

Device-resident x and y, MSM_AMD_SCALAR_MONT_LE, n_rows = n_cols = 2^16, 2^20, 2^22, two seeded shapes of
tests/matvec_ref.py: r1cs (row lengths of mean 3, one row in a thousand of 1 000 entries, one row of n / 4, nine values in
ten +-1, column 0 in a fifth of the rows) and uniform (8 random-valued entries per row); and `witness`, the three stacked
r1cs matrices [A; B; C] of the INTEGRATION recipe at 2^20 as one call.  The clock is pre-warmed as in tools/fr_bench.py;
each row is the median of --iters timed calls after --warmup more: kernel_ms as the call reports it and the wall time of
the blocking call.  The baseline is the host twin at 16 threads on the same box.  Bounds per row:
  hbm     the bytes that must move once -- the matrix (its one allocation: 4 (n_rows + 1) + 8 nnz + 32 per dictionary record + the segment tables), x (32 n_cols) and y
          (32 n_rows) -- over 8 TB/s; the gathered x bytes (32 nnz, what the lanes ask for, mostly from cache) are counted
          beside it as gather_ms at the same rate
  issue   VALU per entry x nnz (+ one store per row) over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles at the clock the run
          reports, VALU = products x 350 + operand loads x 120 + additions x 40 (the weights of tools/fr_bench.py): one
          product, two operand loads (dictionary record, x record) and one addition per entry
Before the rows, the two forms of the kernels -- plain products, and MSM_AMD_FR_MAT_SIGNS=1 -- are timed on the r1cs and
the uniform matrix at 2^20 on a ctx each, alternating --ab-rounds (4) times in the same run (signs_ab in the output).
Writes profiles/matvec_bench.json.

  python tools/matvec_bench.py [--iters 20] [--warmup 3] [--out profiles/matvec_bench.json]

--sweep times the r1cs shape at 2^20 for MSM_AMD_FR_MAT_LONG in {8, 16, 32, 64, 128} x MSM_AMD_FR_MAT_SEG_LOG in {8, 10,
12, 14}, every pair on a ctx of its own, the whole grid --rounds (2) times over in one run so that the spread of a pair
shows beside the differences between pairs, and writes one line per measurement to profiles/fr_mat_ab.txt.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matvec_ref  # noqa: E402
from ntt_bench import HBM_BYTES_PER_S, LANES_PER_CYCLE, commit, shader_clock_mhz  # noqa: E402

LOGS = (16, 20, 22)
SWEEP_LONG, SWEEP_SEG_LOG = (8, 16, 32, 64, 128), (8, 10, 12, 14)


def witness_shape(n):
    """[A; B; C]: three r1cs matrices of n rows over the same n columns, one under the other"""
    parts = [matvec_ref.r1cs_shape(31 + k, n) for k in range(3)]
    row_ptr, base = [np.zeros(1, dtype=np.uint64)], 0
    for p in parts:
        row_ptr.append(p.row_ptr[1:] + np.uint64(base))
        base += p.nnz
    return matvec_ref.Csr(3 * n, n, np.concatenate(row_ptr), np.concatenate([p.col_idx for p in parts]),
                          b"".join(p.values for p in parts))


def make(shape, n):
    return {"r1cs": lambda: matvec_ref.r1cs_shape(3, n), "uniform": lambda: matvec_ref.uniform_shape(4, n),
            "witness": lambda: witness_shape(n)}[shape]()


def timed(cfg, call, warmup, iters):
    for _ in range(warmup):
        call()
    clk = shader_clock_mhz(cfg.device())
    kernel, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        kernel.append(call())
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(kernel), statistics.median(wall), min(kernel), max(kernel), clk


def prewarm(call, ms):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        call()


def sweep(pkg, args):
    n = 1 << args.sweep_log
    mat = make("r1cs", n)
    x = np.random.default_rng(9).bytes(32 * n)
    expect = pkg.host_fr_matvec(*mat.c_args(), x, threads=16)
    lines = []
    for rnd in range(args.rounds):
        for long_rows in SWEEP_LONG:
            for seg_log in SWEEP_SEG_LOG:
                os.environ["MSM_AMD_FR_MAT_LONG"], os.environ["MSM_AMD_FR_MAT_SEG_LOG"] = str(long_rows), str(seg_log)
                cfg = pkg.setup_metal_state(0)
                try:
                    h = cfg.fr_matrix_build(*mat.c_args())
                    d_x, d_y = cfg.alloc(32 * n), cfg.alloc(32 * n)
                    cfg.to_device(d_x, x)
                    call = lambda: cfg.fr_matvec_device(h, d_x, d_y)   # noqa: E731
                    if not lines:
                        prewarm(call, args.prewarm_ms)
                    k_ms, w_ms, k_min, k_max, clk = timed(cfg, call, args.warmup, args.iters)
                    if cfg.to_host(d_y, 32 * n) != expect:
                        raise SystemExit(f"matvec_bench.py: GPU and host twin differ at LONG={long_rows} SEG_LOG={seg_log}")
                    plan = pkg.test_fr_matrix_plan(mat.row_ptr.tobytes(), long_rows, seg_log)
                    plan.pop("segs")
                    lines.append("LONG=%d SEG_LOG=%d round=%d %s" % (long_rows, seg_log, rnd, json.dumps({
                        "shape": "r1cs", "log_n": args.sweep_log, "nnz": mat.nnz, "kernel_ms": round(k_ms, 4),
                        "kernel_min_ms": round(k_min, 4), "kernel_max_ms": round(k_max, 4), "wall_ms": round(w_ms, 4),
                        "sclk_mhz": clk, **plan})))
                    print(lines[-1], flush=True)
                    h.free()
                    cfg.free(d_x)
                    cfg.free(d_y)
                finally:
                    cfg.close()
    os.makedirs(os.path.dirname(args.sweep_out), exist_ok=True)
    with open(args.sweep_out, "w") as f:
        f.write("# tools/matvec_bench.py --sweep on %s: median of %d calls after %d, %d rounds over the grid in one run\n"
                % (socket.gethostname(), args.iters, args.warmup, args.rounds))
        f.write("\n".join(lines) + "\n")


def signs_ab(pkg, args):
    """The two forms of the kernels on the same matrices in one run, alternating: plain products, and
    MSM_AMD_FR_MAT_SIGNS=1 (values 1 and r - 1 added and subtracted without a product); a ctx each."""
    out = []
    for shape in ("r1cs", "uniform"):
        n = 1 << args.sweep_log
        mat = make(shape, n)
        x = np.random.default_rng(9).bytes(32 * n)
        expect = pkg.host_fr_matvec(*mat.c_args(), x, threads=16)
        forms = {}
        for signs in (0, 1):
            os.environ["MSM_AMD_FR_MAT_SIGNS"] = str(signs)
            cfg = pkg.setup_metal_state(0)
            h = cfg.fr_matrix_build(*mat.c_args())
            d_x, d_y = cfg.alloc(32 * n), cfg.alloc(32 * n)
            cfg.to_device(d_x, x)
            forms[signs] = (cfg, (lambda cfg=cfg, h=h, d_x=d_x, d_y=d_y: cfg.fr_matvec_device(h, d_x, d_y)), d_y)
        prewarm(forms[0][1], args.prewarm_ms)
        medians = {0: [], 1: []}
        for _ in range(args.ab_rounds):
            for signs in (0, 1):
                cfg, call, d_y = forms[signs]
                medians[signs].append(round(timed(cfg, call, args.warmup, args.iters)[0], 4))
                if cfg.to_host(d_y, 32 * n) != expect:
                    raise SystemExit(f"matvec_bench.py: GPU and host twin differ: {shape}, signs={signs}")
        for cfg, _, _ in forms.values():
            cfg.close()
        plain, signed = medians[0], medians[1]
        row = {"shape": shape, "log_n": args.sweep_log, "nnz": mat.nnz, "products_kernel_ms": plain, "signs_kernel_ms": signed,
               "products_median_ms": round(statistics.median(plain), 4), "signs_median_ms": round(statistics.median(signed), 4),
               "products_spread_ms": round(max(plain) - min(plain), 4),
               "signs_gain_ms": round(statistics.median(plain) - statistics.median(signed), 4)}
        row["signs_wins"] = row["signs_gain_ms"] > row["products_spread_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--witness-log", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-log", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ab-rounds", type=int, default=4, help="alternations of the two kernel forms (0: skip the comparison)")
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "fr_mat_ab.txt"))
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matvec_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("matvec_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    if args.sweep:
        return sweep(pkg, args)
    ab = signs_ab(pkg, args) if args.ab_rounds else None
    os.environ.pop("MSM_AMD_FR_MAT_SIGNS", None)
    cfg = pkg.setup_metal_state(0)
    rows, clocks = [], []
    try:
        for shape, log_n in [(s, l) for l in args.logs for s in ("r1cs", "uniform")] + [("witness", args.witness_log)]:
            n = 1 << log_n
            mat = make(shape, n)
            x = np.random.default_rng(9).bytes(32 * n)                       # any 256-bit word is a record
            t0 = time.perf_counter()
            h = cfg.fr_matrix_build(*mat.c_args())
            build_ms = (time.perf_counter() - t0) * 1e3
            info = h.info()
            d_x, d_y = cfg.alloc(32 * n), cfg.alloc(32 * mat.n_rows)
            cfg.to_device(d_x, x)
            call = lambda: cfg.fr_matvec_device(h, d_x, d_y)   # noqa: E731
            if not rows:
                prewarm(call, args.prewarm_ms)
            k_ms, w_ms, k_min, k_max, clk = timed(cfg, call, args.warmup, args.iters)
            got = cfg.to_host(d_y, 32 * mat.n_rows)
            host_ms = []
            for _ in range(args.host_iters):
                t0 = time.perf_counter()
                ref = pkg.host_fr_matvec(*mat.c_args(), x, threads=16)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            if ref != got:
                raise SystemExit(f"matvec_bench.py: GPU and host twin differ: {shape} at log_n={log_n}")
            h_ms = statistics.median(host_ms)
            mhz = clk or args.nominal_mhz
            nnz = mat.nnz
            matrix_bytes = info["device_bytes"]                              # offsets, entries, dictionary, segment tables
            x_bytes, gathered_bytes, y_bytes = 32 * n, 32 * nnz, 32 * mat.n_rows
            valu = nnz * (args.valu_per_product + 2 * args.valu_per_load + args.valu_per_add) + mat.n_rows * args.valu_per_load
            hbm_ms = (matrix_bytes + x_bytes + y_bytes) / HBM_BYTES_PER_S * 1e3
            gather_ms = gathered_bytes / HBM_BYTES_PER_S * 1e3
            issue_ms = valu / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
            clocks.append(clk)
            rows.append({
                "shape": shape, "log_n": log_n, "n_rows": mat.n_rows, "n_cols": n, "nnz": nnz,
                "n_distinct": info["n_distinct"], "device_bytes": info["device_bytes"], "build_ms": round(build_ms, 1),
                "kernel_ms": round(k_ms, 4), "kernel_min_ms": round(k_min, 4), "kernel_max_ms": round(k_max, 4),
                "wall_ms": round(w_ms, 4), "host_gap_ms": round(w_ms - k_ms, 4),
                "host_twin_16_threads_ms": round(h_ms, 2), "speedup_over_host": round(h_ms / w_ms, 1),
                "sclk_mhz": clk, "products_per_nnz": 1, "matrix_bytes": matrix_bytes, "x_bytes": x_bytes,
                "gathered_x_bytes": gathered_bytes, "y_bytes": y_bytes,
                "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
                "gather_ms": round(gather_ms, 4), "gather_fraction": round(gather_ms / k_ms, 3),
                "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
                "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
                "nnz_per_us": round(nnz / k_ms / 1e3, 1),
            })
            print(json.dumps(rows[-1]), flush=True)
            h.free()
            cfg.free(d_x)
            cfg.free(d_y)
            del mat, x, got, ref
    finally:
        cfg.close()
    result = {
        "tool": "tools/matvec_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add,
        "knobs": {"MSM_AMD_FR_MAT_LONG": os.environ.get("MSM_AMD_FR_MAT_LONG", "default"),
                  "MSM_AMD_FR_MAT_SEG_LOG": os.environ.get("MSM_AMD_FR_MAT_SEG_LOG", "default")},
        "setting": "device-resident x and y, MONT_LE; median of the timed calls; host = the twin at 16 threads",
        "rows": rows,
        "signs_ab": ab,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
