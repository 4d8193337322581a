#!/usr/bin/env python3
"""Time the polynomial calls over Fr on one GPU against their host twins.

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, out of place, sizes 2^16, 2^20, 2^24: poly_eval, poly_div_linear (with
its remainder), lincomb of --n-vec (8) vectors of n, and -- same run, same build, same n -- the prefix product, whose
kernels the division is held against (div_over_prefix: the ratio of the two kernel_ms of a size).  The clock is pre-warmed
as in tools/fr_bench.py; each row is the median of --iters timed calls after --warmup more: kernel_ms as the call reports it
and the wall time of the blocking call (which holds the one copy of the values and the one wait).  The baseline is the
host twin at 16 threads on the same box.  Bounds per row, per element of n (lincomb: per output element):
  hbm    bytes read + written x n over 8 TB/s
  issue  VALU per element x n over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles at the clock the run reports, VALU = products x
         350 + operand loads x 120 + additions x 40 (the weights of tools/fr_bench.py) with the counted products of DESIGN.md
         section 8.7: 1 + 6/per (evaluation), (1 + 6/per) + (2 + 6/per) (division), n_vec - 1 (fold); one addition per product
Writes profiles/poly_bench.json.

  python tools/poly_bench.py [--iters 20] [--warmup 3] [--host-iters 1] [--out profiles/poly_bench.json]
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
OPS = ("prefix_product", "poly_eval", "poly_div_linear", "lincomb")


def counted(tile_log, n_vec):
    """per element: (products, operand loads, additions, HBM bytes)"""
    per = float(1 << max(0, tile_log - 6))
    red, scan = 1 + 6 / per, 2 + 6 / per
    return {"prefix_product": (red + scan, 2, 0, 96), "poly_eval": (red, 1, red, 32),
            "poly_div_linear": (red + scan, 2, red + scan, 96), "lincomb": (n_vec - 1, n_vec, n_vec - 1, 32 * (n_vec + 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--n-vec", type=int, default=8, help="vectors of the fold")
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--tile-log", type=int, default=int(os.environ.get("MSM_AMD_FR_TILE_LOG", "9")),
                    help="the tile the library runs with (MSM_AMD_FR_TILE_LOG): only the counted products depend on it")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("poly_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    z = (12345).to_bytes(32, "little")
    n_vec = args.n_vec
    COUNTED = counted(max(2, min(9, args.tile_log)), n_vec)
    rows, clocks = [], []
    try:
        for log_n in args.logs:
            n = 1 << log_n
            nbytes = 32 * n
            raw = np.random.default_rng(7).integers(0, 256, size=nbytes, dtype=np.uint8)
            raw[31::32] &= 0x1F                                              # every record < 2^253 < r
            a = raw.tobytes()
            vecs = a * n_vec                                                 # the fold's vectors: n_vec copies of a
            d_in, d_vecs, d_out = cfg.alloc(nbytes), cfg.alloc(nbytes * n_vec), cfg.alloc(nbytes)
            cfg.to_device(d_in, a)
            cfg.to_device(d_vecs, vecs)
            last = {}

            def dev_eval():
                last["values"], ms = cfg.fr_poly_eval_device(d_in, n, z)
                return ms

            def dev_div():
                last["values"], ms = cfg.fr_poly_div_linear_device(d_in, n, d_out, z)
                return ms

            device = {"prefix_product": lambda: cfg.fr_prefix_product_device(d_in, n, d_out), "poly_eval": dev_eval,
                      "poly_div_linear": dev_div, "lincomb": lambda: cfg.fr_lincomb_device(d_vecs, n, d_out, z, n_vec=n_vec)}
            host = {"prefix_product": lambda: (pkg.host_fr_prefix_product(a, threads=16), None),
                    "poly_eval": lambda: (b"", pkg.host_fr_poly_eval(a, z, threads=16)),
                    "poly_div_linear": lambda: pkg.host_fr_poly_div_linear(a, z, threads=16),
                    "lincomb": lambda: (pkg.host_fr_lincomb(vecs, z, n_vec=n_vec, threads=16), None)}
            if not rows:                                                     # pre-warm once, on the first size's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    device["poly_div_linear"]()
            by_op = {}
            for op in OPS:
                for _ in range(args.warmup):
                    device[op]()
                clk = shader_clock_mhz(cfg.device())
                kernel, wall = [], []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    kernel.append(device[op]())
                    wall.append((time.perf_counter() - t0) * 1e3)
                got = b"" if op == "poly_eval" else cfg.to_host(d_out, min(nbytes, 1 << 20))
                host_ms = []
                for _ in range(args.host_iters):
                    t0 = time.perf_counter()
                    ref, ref_values = host[op]()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                if ref[:len(got)] != got or (ref_values is not None and ref_values != last["values"]):
                    raise SystemExit(f"poly_bench.py: GPU and host twin differ: {op} at log_n={log_n}")
                k_ms, w_ms, h_ms = statistics.median(kernel), statistics.median(wall), statistics.median(host_ms)
                mhz = clk or args.nominal_mhz
                prod, loads, adds, hbm_bytes = COUNTED[op]
                valu = prod * args.valu_per_product + loads * args.valu_per_load + adds * args.valu_per_add
                hbm_ms = hbm_bytes * n / HBM_BYTES_PER_S * 1e3
                issue_ms = valu * n / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
                clocks.append(clk)
                by_op[op] = k_ms
                rows.append({
                    "op": op, "log_n": log_n, "n_vec": n_vec if op == "lincomb" else 1,
                    "kernel_ms": round(k_ms, 4), "wall_ms": round(w_ms, 4), "host_gap_ms": round(w_ms - k_ms, 4),
                    "host_twin_16_threads_ms": round(h_ms, 2), "speedup_over_host": round(h_ms / w_ms, 1),
                    "sclk_mhz": clk, "products_per_element": prod, "valu_per_element": valu,
                    "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
                    "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
                    "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
                })
                if op == "poly_div_linear":
                    rows[-1]["div_over_prefix"] = round(k_ms / by_op["prefix_product"], 3)
                print(json.dumps(rows[-1]), flush=True)
            for d in (d_in, d_vecs, d_out):
                cfg.free(d)
    finally:
        cfg.close()
    result = {
        "tool": "tools/poly_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add, "tile_log": args.tile_log, "n_vec": n_vec,
        "setting": "device-resident, MONT_LE, out of place; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
