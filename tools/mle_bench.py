#!/usr/bin/env python3
"""Time the multilinear calls over Fr on one GPU against their host twins and against the kernels they are held to
(DESIGN.md section 8.9).

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, n = 2^16, 2^20, 2^24: mle_bind of one variable (both orders) and of three,
mle_eval, eq_table, and a sumcheck round of PRODUCT over two tables and of EQ_AB_C -- and, same run, same build, the calls
they are compared with: MSM_AMD_FR_MUL at n/2 records (bind), poly_eval at n (eval), MSM_AMD_FR_MULSUB_SCALE at n/2 records
(round).  The clock is pre-warmed as in tools/fr_bench.py; each row is the median of --iters timed calls after --warmup
more: kernel_ms as the call reports it and the wall time of the blocking call.  The baseline is the host twin at 16 threads
on the same box (up to --host-max-log; the values of a round and of an evaluation must equal the twin's).  Bounds per row,
per element (a pair of a round, an output of a bind or of the eq table, a record of an evaluation):
  hbm    bytes read + written x elements over 8 TB/s
  issue  VALU per element x elements over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles at the clock the run reports, VALU =
         products x 350 + operand loads x 120 + additions x 40 (the weights of tools/fr_bench.py)
--sweep LOG ..: the rounds once more on a fresh ctx per MSM_AMD_FR_MLE_CHUNK_LOG, written to --sweep-out as text.
Writes profiles/mle_bench.json.

  python tools/mle_bench.py [--iters 20] [--warmup 3] [--sweep 6 8 10 12 14] [--out profiles/mle_bench.json]
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
from ntt_bench import HBM_BYTES_PER_S, LANES_PER_CYCLE, commit, shader_clock_mhz  # noqa: E402

LOGS = (16, 20, 24)
# per element: (products, operand loads, additions, HBM bytes); eq_table is filled in per m
COUNTED = {
    "mle_bind_high_1": (1, 2, 2, 96), "mle_bind_low_1": (1, 2, 2, 96), "mle_bind_high_3": (7, 8, 14, 288),
    "mle_eval": (1, 1, 2, 32), "round_product_2": (3, 4, 9, 128), "round_eq_ab_c": (8, 8, 24, 256),
    "fr_mul_half": (1, 2, 0, 96), "poly_eval": (1.75, 1, 1.75, 32), "fr_mulsub_scale_half": (3, 3, 1, 128),
}
HELD_TO = {"mle_bind_high_1": ("fr_mul_half", 1.25), "mle_bind_low_1": ("fr_mul_half", 1.25), "mle_eval": ("poly_eval", 1.25),
           "round_product_2": ("fr_mulsub_scale_half", 1.65 * 1.25), "round_eq_ab_c": ("fr_mulsub_scale_half", 4.3 * 1.25)}
GATED_LOGS = {"mle_bind_high_1": (20, 24), "mle_bind_low_1": (20, 24), "mle_eval": (20, 24), "round_product_2": (24,),
              "round_eq_ab_c": (24,)}


def table(n, seed=7):
    raw = np.random.default_rng(seed).integers(0, 256, size=32 * n, dtype=np.uint8)
    raw[31::32] &= 0x1F                                                  # every record < 2^253 < r
    return raw.tobytes()


def median_ms(call, warmup, iters):
    for _ in range(warmup):
        call()
    kernel, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        kernel.append(call())
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(kernel), statistics.median(wall)


def sweep(pkg, args):
    """the two gated rounds at every chunk log of the sweep, a fresh ctx each"""
    lines = ["# tools/mle_bench.py --sweep: kernel_ms of msm_amd_fr_sumcheck_round_device, MONT_LE, HIGH; median of %d after %d"
             % (args.iters, args.warmup), "# chunk_log  log_n  form          launches  kernel_ms"]
    best = {}
    for log_n in (20, 24):
        n = 1 << log_n
        a = table(n)
        for chunk_log in args.sweep:
            os.environ["MSM_AMD_FR_MLE_CHUNK_LOG"] = str(chunk_log)
            cfg = pkg.setup_metal_state(0)
            try:
                d_in = cfg.alloc(32 * n * 4)
                for v in range(4):
                    cfg.to_device(d_in + 32 * n * v, a)
                for name, form, k in (("product_2", pkg.SUMCHECK_PRODUCT, 2), ("eq_ab_c", pkg.SUMCHECK_EQ_AB_C, 4)):
                    k_ms, _ = median_ms(lambda: cfg.fr_sumcheck_round_device(d_in, n, form, pkg.MLE_HIGH, n_vec=k)[1],
                                        args.warmup, args.iters)
                    launches = pkg.test_fr_mle_plan(pkg.MLE_CALL_ROUND, n, k, form=form, chunk_log=chunk_log)["launches"]
                    lines.append("%-11d %-6d %-13s %-9d %.4f" % (chunk_log, log_n, name, launches, k_ms))
                    best.setdefault((log_n, name), []).append((k_ms, chunk_log))
                    print(lines[-1], flush=True)
                cfg.free(d_in)
            finally:
                cfg.close()
    os.environ.pop("MSM_AMD_FR_MLE_CHUNK_LOG", None)
    for (log_n, name), got in sorted(best.items()):
        lines.append("# fastest at 2^%d %s: chunk_log %d" % (log_n, name, min(got)[1]))
    os.makedirs(os.path.dirname(args.sweep_out), exist_ok=True)
    with open(args.sweep_out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-max-log", type=int, default=20, help="the host twins run up to this size")
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--sweep", type=int, nargs="*", default=[], help="chunk logs of the round to sweep first")
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "mle_ab.txt"))
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("mle_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    if args.sweep:
        sweep(pkg, args)
    cfg = pkg.setup_metal_state(0)
    HIGH, LOW = pkg.MLE_HIGH, pkg.MLE_LOW
    z = (12345).to_bytes(32, "little")
    rows, clocks = [], []
    try:
        for log_n in args.logs:
            n = 1 << log_n
            a = table(n)
            point = table(log_n, 11)
            d_in, d_out = cfg.alloc(32 * n * 4), cfg.alloc(32 * n)
            for v in range(4):
                cfg.to_device(d_in + 32 * n * v, a)
            last = {}

            def values(call):
                last["values"], ms = call()
                return ms

            device = {
                "fr_mul_half": lambda: cfg.fr_map_device(pkg.FR_MUL, d_in, d_in + 32 * n, None, n // 2, d_out),
                "mle_bind_high_1": lambda: cfg.fr_mle_bind_device(d_in, n, d_out, point[:32], HIGH),
                "mle_bind_low_1": lambda: cfg.fr_mle_bind_device(d_in, n, d_out, point[:32], LOW),
                "mle_bind_high_3": lambda: cfg.fr_mle_bind_device(d_in, n, d_out, point[:96], HIGH),
                "poly_eval": lambda: values(lambda: cfg.fr_poly_eval_device(d_in, n, z)),
                "mle_eval": lambda: values(lambda: cfg.fr_mle_eval_device(d_in, n, point, HIGH)),
                "eq_table": lambda: cfg.fr_eq_table_device(d_out, point, HIGH),
                "fr_mulsub_scale_half": lambda: cfg.fr_map_device(pkg.FR_MULSUB_SCALE, d_in, d_in + 32 * n, d_in + 64 * n, n // 2,
                                                                  d_out, k=z),
                "round_product_2": lambda: values(lambda: cfg.fr_sumcheck_round_device(d_in, n, pkg.SUMCHECK_PRODUCT, HIGH, n_vec=2)),
                "round_eq_ab_c": lambda: values(lambda: cfg.fr_sumcheck_round_device(d_in, n, pkg.SUMCHECK_EQ_AB_C, HIGH, n_vec=4)),
            }
            host = {
                "mle_bind_high_1": lambda: (pkg.host_fr_mle_bind(a, point[:32], n, HIGH, threads=16), None),
                "mle_bind_low_1": lambda: (pkg.host_fr_mle_bind(a, point[:32], n, LOW, threads=16), None),
                "mle_bind_high_3": lambda: (pkg.host_fr_mle_bind(a, point[:96], n, HIGH, threads=16), None),
                "mle_eval": lambda: (b"", pkg.host_fr_mle_eval(a, point, n, HIGH, threads=16)),
                "eq_table": lambda: (pkg.host_fr_eq_table(point, HIGH, threads=16), None),
                "round_product_2": lambda: (b"", pkg.host_fr_sumcheck_round(a * 2, n, pkg.SUMCHECK_PRODUCT, HIGH, n_vec=2, threads=16)),
                "round_eq_ab_c": lambda: (b"", pkg.host_fr_sumcheck_round(a * 4, n, pkg.SUMCHECK_EQ_AB_C, HIGH, n_vec=4, threads=16)),
            }
            counted = dict(COUNTED, eq_table=((log_n + 10) / 8.0, 0, 0, 32))
            out_records = {"mle_bind_high_1": n // 2, "mle_bind_low_1": n // 2, "mle_bind_high_3": n // 8, "eq_table": n}
            elements = {"mle_bind_high_3": n // 8, "mle_eval": n, "poly_eval": n, "eq_table": n}
            if not rows:                                                     # pre-warm once, on the first size's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    device["round_eq_ab_c"]()
            by_op = {}
            for op in device:
                k_ms, w_ms = median_ms(device[op], args.warmup, args.iters)
                clk = shader_clock_mhz(cfg.device())
                h_ms = None
                if op in host and log_n <= args.host_max_log:
                    got = cfg.to_host(d_out, 32 * min(out_records[op], 1 << 15)) if op in out_records else b""
                    t0 = time.perf_counter()
                    ref, ref_values = host[op]()
                    h_ms = (time.perf_counter() - t0) * 1e3
                    if ref[:len(got)] != got or (ref_values is not None and ref_values != last["values"]):
                        raise SystemExit(f"mle_bench.py: GPU and host twin differ: {op} at log_n={log_n}")
                mhz = clk or args.nominal_mhz
                prod, loads, adds, hbm_bytes = counted[op]
                count = elements.get(op, n // 2)
                valu = prod * args.valu_per_product + loads * args.valu_per_load + adds * args.valu_per_add
                hbm_ms = hbm_bytes * count / HBM_BYTES_PER_S * 1e3
                issue_ms = valu * count / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
                clocks.append(clk)
                by_op[op] = k_ms
                rows.append({
                    "op": op, "log_n": log_n, "elements": count,
                    "kernel_ms": round(k_ms, 4), "wall_ms": round(w_ms, 4), "host_gap_ms": round(w_ms - k_ms, 4),
                    "host_twin_16_threads_ms": None if h_ms is None else round(h_ms, 2),
                    "speedup_over_host": None if h_ms is None else round(h_ms / w_ms, 1),
                    "sclk_mhz": clk, "products_per_element": prod, "valu_per_element": valu,
                    "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
                    "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
                    "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
                })
                if op in HELD_TO:
                    ref_op, bound = HELD_TO[op]
                    rows[-1]["held_to"] = ref_op
                    rows[-1]["ratio"] = round(k_ms / by_op[ref_op], 3)
                    if log_n in GATED_LOGS[op]:
                        rows[-1]["ratio_bound"] = round(bound, 3)
                        rows[-1]["within_bound"] = bool(k_ms / by_op[ref_op] <= bound)
                print(json.dumps(rows[-1]), flush=True)
            cfg.free(d_in)
            cfg.free(d_out)
    finally:
        cfg.close()
    result = {
        "tool": "tools/mle_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add, "chunk_log": int(os.environ.get("MSM_AMD_FR_MLE_CHUNK_LOG", "0")) or "default",
        "setting": "device-resident, MONT_LE, out of place, HIGH unless the row says LOW; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
