#!/usr/bin/env python3
"""Time the multi-point polynomial calls over Fr on one GPU against the chains of single-point calls they replace
(DESIGN.md section 8.18).

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, sizes 2^16, 2^20, 2^24, k = 2, 3, 5 points, one polynomial:
  div_points   msm_amd_fr_poly_div_points (with its values), out of place, against the chain of k
               msm_amd_fr_poly_div_linear_device calls (the first out of place, the others in place on its output: upstream's
               roots.iter().fold(poly, kate_division))
  eval_points  msm_amd_fr_poly_eval_points against k msm_amd_fr_poly_eval_device calls
Both sides of a row are timed in the same run and build.  The clock is pre-warmed as in tools/fr_bench.py; each figure is the
median of --iters timed calls after --warmup more: kernel_ms as the calls report it (summed over a chain) and the wall time
of the blocking call or chain.  The fused result is compared with the chain's in bytes.  Bounds per row, per record of n:
  hbm    bytes read + written x n over 8 TB/s
  issue  VALU per record x n over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles at the clock the run reports, VALU = products x 350
         + operand loads x 120 + additions x 40 (the weights of tools/fr_bench.py) with the counted products of DESIGN.md
         section 8.18: k (1 + 6/per) (evaluation), k (3 + 12/per) + k - 1 (division); a chain: k times the single-point call
Writes profiles/multiopen_bench.json.

  python tools/multiopen_bench.py [--iters 20] [--warmup 3] [--out profiles/multiopen_bench.json]
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
KS = (2, 3, 5)
MARGIN = 1.25     # the project's usual margin over a ratio of counted products


def counted(tile_log, k):
    """per record: op -> (products, operand loads, additions, HBM bytes), the fused call and its chain"""
    per = float(1 << max(0, tile_log - 6))
    red, scan = 1 + 6 / per, 2 + 6 / per
    return {
        "eval_points": ((k * red, 1, k * red, 32), (k * red, k, k * red, 32 * k)),
        "div_points": ((k * (red + scan) + k - 1, 2, k * (red + scan) + 2 * (k - 1), 96),
                       (k * (red + scan), 2 * k, k * (red + scan), 96 * k)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--logs", type=int, nargs="*", default=list(LOGS))
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--tile-log", type=int, default=int(os.environ.get("MSM_AMD_FR_TILE_LOG", "9")),
                    help="the tile the library runs with (MSM_AMD_FR_TILE_LOG): only the counted products depend on it")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiopen_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("multiopen_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    mem = pkg.MEM_DEVICE
    rows, clocks = [], []

    def timed(fn):
        """(median kernel_ms, median wall ms, the clock before the timed calls)"""
        for _ in range(args.warmup):
            fn()
        clk = shader_clock_mhz(cfg.device())
        kernel, wall = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            kernel.append(fn())
            wall.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(kernel), statistics.median(wall), clk

    try:
        for log_n in args.logs:
            n = 1 << log_n
            nbytes = 32 * n
            raw = np.random.default_rng(7).integers(0, 256, size=nbytes, dtype=np.uint8)
            raw[31::32] &= 0x1F                                              # every record < 2^253 < r
            d_in, d_out, d_chain = cfg.alloc(nbytes), cfg.alloc(nbytes), cfg.alloc(nbytes)
            cfg.to_device(d_in, raw.tobytes())
            for k in args.ks:
                points = [(12345 + 1000003 * j).to_bytes(32, "little") for j in range(k)]
                z = b"".join(points)
                last = {}

                def fused_div():
                    _, last["fused"], ms = cfg.fr_poly_div_points(d_in, z, n_vec=1, mem=mem, n=n, out=d_out)
                    return ms

                def chain_div():
                    total, vals = 0.0, []
                    for j, zj in enumerate(points):
                        rem, ms = cfg.fr_poly_div_linear_device(d_in if j == 0 else d_chain, n, d_chain, zj)
                        total += ms
                        vals.append(rem)
                    last["chain"] = vals
                    return total

                def fused_eval():
                    last["fused"], ms = cfg.fr_poly_eval_points(d_in, z, n_vec=1, mem=mem, n=n)
                    return ms

                def chain_eval():
                    total, vals = 0.0, []
                    for zj in points:
                        y, ms = cfg.fr_poly_eval_device(d_in, n, zj)
                        total += ms
                        vals.append(y)
                    last["chain"] = b"".join(vals)
                    return total

                if not rows:                                                 # pre-warm once, on the first size's load
                    t0 = time.perf_counter()
                    while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                        fused_div()
                for op, fused, chain in (("div_points", fused_div, chain_div), ("eval_points", fused_eval, chain_eval)):
                    ck_ms, cw_ms, _ = timed(chain)
                    fk_ms, fw_ms, clk = timed(fused)
                    if op == "div_points":
                        head = min(nbytes, 1 << 20)
                        if cfg.to_host(d_out, head) != cfg.to_host(d_chain, head) or \
                                cfg.to_host(d_out + nbytes - head, head) != cfg.to_host(d_chain + nbytes - head, head):
                            raise SystemExit(f"multiopen_bench.py: the fused quotient differs from the chain's: k={k} log_n={log_n}")
                        # the chain's j-th remainder is the value of the j-th partial quotient: only the first is p(z_0)
                        if last["fused"][:32] != last["chain"][0]:
                            raise SystemExit(f"multiopen_bench.py: p(z_0) differs: k={k} log_n={log_n}")
                    elif last["fused"] != last["chain"]:
                        raise SystemExit(f"multiopen_bench.py: the fused values differ from the chain's: k={k} log_n={log_n}")
                    mhz = clk or args.nominal_mhz
                    clocks.append(clk)
                    (prod, loads, adds, hbm_bytes), (c_prod, c_loads, c_adds, c_hbm) = counted(max(2, min(9, args.tile_log)), k)[op]
                    valu = prod * args.valu_per_product + loads * args.valu_per_load + adds * args.valu_per_add
                    c_valu = c_prod * args.valu_per_product + c_loads * args.valu_per_load + c_adds * args.valu_per_add
                    per_ms = n / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
                    hbm_ms, issue_ms = hbm_bytes * n / HBM_BYTES_PER_S * 1e3, valu * per_ms
                    rows.append({
                        "op": op, "log_n": log_n, "k": k, "sclk_mhz": clk,
                        "kernel_ms": round(fk_ms, 4), "wall_ms": round(fw_ms, 4),
                        "chain_kernel_ms": round(ck_ms, 4), "chain_wall_ms": round(cw_ms, 4),
                        "kernel_ratio": round(fk_ms / ck_ms, 3), "wall_ratio": round(fw_ms / cw_ms, 3),
                        "products_per_record": prod, "chain_products_per_record": c_prod,
                        "product_ratio": round(prod / c_prod, 3), "bar": round(prod / c_prod * MARGIN, 3),
                        "valu_per_record": valu, "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / fk_ms, 3),
                        "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / fk_ms, 3),
                        "chain_issue_fraction": round(c_valu * per_ms / ck_ms, 3),
                        "chain_hbm_fraction": round(c_hbm * n / HBM_BYTES_PER_S * 1e3 / ck_ms, 3),
                        "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
                    })
                    print(json.dumps(rows[-1]), flush=True)
            for d in (d_in, d_out, d_chain):
                cfg.free(d)
    finally:
        cfg.close()
    result = {
        "tool": "tools/multiopen_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add, "tile_log": args.tile_log, "margin": MARGIN,
        "setting": "device-resident, MONT_LE, one polynomial, out of place; median of the timed calls; the chain in the same run",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
