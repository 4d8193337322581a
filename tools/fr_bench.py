#!/usr/bin/env python3
"""Time the Fr vector calls on one GPU against their host twins.

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, out of place, sizes 2^16, 2^20, 2^24; ops ADD, MUL, MULSUB_SCALE,
batch_inverse, prefix_product (inclusive).  The clock is pre-warmed the way bench.py does it (untimed calls of the same
load before anything is counted); each row is the median of --iters timed calls after --warmup more: kernel_ms as the
call reports it (the events round the kernels; the inversion: the sum of its two spans) and the wall time of the blocking
call -- for the inversion the difference holds the copy of T, the host's Fermat inversion and the second wait.  The
baseline is the host twin at 16 threads on the same box.  Bounds per row:
  hbm    bytes read + written per element (HBM_BYTES) x n over 8 TB/s
  issue  VALU instructions per element x n lane-instructions over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles (the project's
         measured rate of one wave-instruction per ~4 cycles per SIMD) at the clock the run reports.
         VALU per element = products x --valu-per-product + loads x --valu-per-load + adds x --valu-per-add, with the
         counted products per element of DESIGN.md section 8.6 (PRODUCTS) and k_fr.s behind the three weights: 350 VALU
         per Montgomery product, 120 per operand load (five conditional subtractions of eight limbs), 40 per addition
Writes profiles/fr_bench.json.

  python tools/fr_bench.py [--iters 20] [--warmup 3] [--host-iters 1] [--out profiles/fr_bench.json]
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
OPS = ("add", "mul", "mulsub_scale", "batch_inverse", "prefix_product")


def products(tile_log):
    """A tile of 2^T records is one wave: per = 2^(T - 6) records per lane, six shuffle steps per scan of the lane products.
    prefix_product: 1 + 6/per in the reduction, 2 + 6/per in the scan (the totals' own scan: 2^-T of that).
    batch_inverse (tiles of 2^min(T, 8)): 1 + 6/per in the reduction; 1 + 2 + (6 + 6 + 4)/per in the last kernel."""
    per, per_inv = float(1 << max(0, tile_log - 6)), float(1 << max(0, min(tile_log, 8) - 6))
    return {"add": 0.0, "mul": 1.0, "mulsub_scale": 2.0, "batch_inverse": (1 + 6 / per_inv) + (3 + 16 / per_inv),
            "prefix_product": (1 + 6 / per) + (2 + 6 / per)}


# per element: operand loads, additions / subtractions, bytes over HBM
LOADS = {"add": 2, "mul": 2, "mulsub_scale": 3, "batch_inverse": 2, "prefix_product": 2}
ADDS = {"add": 1, "mul": 0, "mulsub_scale": 1, "batch_inverse": 0, "prefix_product": 0}
HBM_BYTES = {"add": 96, "mul": 96, "mulsub_scale": 128, "batch_inverse": 96, "prefix_product": 96}


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
    ap.add_argument("--tile-log", type=int, default=int(os.environ.get("MSM_AMD_FR_TILE_LOG", "9")),
                    help="the tile the library runs with (MSM_AMD_FR_TILE_LOG): only the counted products depend on it")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("fr_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    k = (12345).to_bytes(32, "little")
    PRODUCTS = products(max(2, min(9, args.tile_log)))
    rows, clocks = [], []
    try:
        for log_n in args.logs:
            n = 1 << log_n
            nbytes = 32 * n
            host_in, d_in = [], []
            for seed in range(3):
                raw = np.random.default_rng(7 + seed).integers(0, 256, size=nbytes, dtype=np.uint8)
                raw[31::32] &= 0x1F                                          # every record < 2^253 < r
                host_in.append(raw.tobytes())
                d_in.append(cfg.alloc(nbytes))
                cfg.to_device(d_in[-1], host_in[-1])
            d_out = cfg.alloc(nbytes)
            a, b, c = host_in
            device = {
                "add": lambda: cfg.fr_map_device(pkg.FR_ADD, d_in[0], d_in[1], None, n, d_out),
                "mul": lambda: cfg.fr_map_device(pkg.FR_MUL, d_in[0], d_in[1], None, n, d_out),
                "mulsub_scale": lambda: cfg.fr_map_device(pkg.FR_MULSUB_SCALE, d_in[0], d_in[1], d_in[2], n, d_out, k),
                "batch_inverse": lambda: cfg.fr_batch_inverse_device(d_in[0], n, d_out)[1],
                "prefix_product": lambda: cfg.fr_prefix_product_device(d_in[0], n, d_out),
            }
            host = {
                "add": lambda: pkg.host_fr_map(pkg.FR_ADD, a, b, threads=16),
                "mul": lambda: pkg.host_fr_map(pkg.FR_MUL, a, b, threads=16),
                "mulsub_scale": lambda: pkg.host_fr_map(pkg.FR_MULSUB_SCALE, a, b, c, k, threads=16),
                "batch_inverse": lambda: pkg.host_fr_batch_inverse(a, threads=16)[0],
                "prefix_product": lambda: pkg.host_fr_prefix_product(a, threads=16),
            }
            if not rows:                                                     # pre-warm once, on the first size's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    device["mulsub_scale"]()
            for op in OPS:
                for _ in range(args.warmup):
                    device[op]()
                clk = shader_clock_mhz(cfg.device())
                kernel, wall = [], []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    kernel.append(device[op]())
                    wall.append((time.perf_counter() - t0) * 1e3)
                got = cfg.to_host(d_out, min(nbytes, 1 << 20))
                host_ms = []
                for _ in range(args.host_iters):
                    t0 = time.perf_counter()
                    ref = host[op]()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                if ref[:len(got)] != got:
                    raise SystemExit(f"fr_bench.py: GPU and host twin differ: {op} at log_n={log_n}")
                k_ms, w_ms, h_ms = statistics.median(kernel), statistics.median(wall), statistics.median(host_ms)
                mhz = clk or args.nominal_mhz
                valu = (PRODUCTS[op] * args.valu_per_product + LOADS[op] * args.valu_per_load + ADDS[op] * args.valu_per_add)
                hbm_ms = HBM_BYTES[op] * n / HBM_BYTES_PER_S * 1e3
                issue_ms = valu * n / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
                clocks.append(clk)
                rows.append({
                    "op": op, "log_n": log_n, "kernel_ms": round(k_ms, 4), "wall_ms": round(w_ms, 4),
                    "host_gap_ms": round(w_ms - k_ms, 4),
                    "host_twin_16_threads_ms": round(h_ms, 2), "speedup_over_host": round(h_ms / w_ms, 1),
                    "sclk_mhz": clk, "products_per_element": PRODUCTS[op], "valu_per_element": valu,
                    "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
                    "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
                    "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
                })
                print(json.dumps(rows[-1]), flush=True)
            for d in d_in + [d_out]:
                cfg.free(d)
    finally:
        cfg.close()
    result = {
        "tool": "tools/fr_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add, "tile_log": args.tile_log,
        "setting": "device-resident, MONT_LE, out of place; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
