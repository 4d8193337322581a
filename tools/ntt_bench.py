#!/usr/bin/env python3
"""Time the transform on one GPU against the host twin.

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, FORWARD, no shift, out of place.  The clock is pre-warmed the way
bench.py does it (untimed calls of the same load before anything is counted); each row is the median of --iters timed
calls after --warmup more: kernel_ms as the call reports it (two events round the passes) and the wall time of the
blocking call.  The baseline is msm_amd_host_ntt at 16 threads on the same box.  Bounds per row:
  hbm    passes x 64 B x n x n_vec over 8 TB/s (every pass reads and writes the batch once)
  issue  --valu-per-butterfly VALU instructions (counted from k_ntt.s) x (n / 2) log_n n_vec lane-instructions, over
         256 CUs x 4 SIMDs x 64 lanes / 4 cycles (the project's measured rate of one wave-instruction per ~4 cycles per
         SIMD) at the clock the run reports
Writes profiles/ntt_bench.json.

  python tools/ntt_bench.py [--iters 20] [--warmup 3] [--host-iters 1] [--out profiles/ntt_bench.json]
"""
import argparse
import importlib
import json
import os
import re
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = [(16, 1), (20, 1), (24, 1), (20, 8)]   # (log_n, n_vec)
HBM_BYTES_PER_S = 8e12
LANES_PER_CYCLE = 256 * 4 * 64 / 4.0


def shader_clock_mhz(device):
    """rocm-smi asked (read only) while the load runs; None when it cannot be had"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json", "-d", str(device)], capture_output=True, text=True, timeout=20)
        card = next(iter(json.loads(r.stdout).values()))
        clk = re.search(r"(\d+)\s*Mhz", card.get("sclk clock speed:", ""), re.I)
        return int(clk.group(1)) if clk else None
    except Exception:
        return None


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--valu-per-butterfly", type=float, default=530.0,
                    help="VALU instructions of one butterfly in the two-level step of ntt_pass_kernel (k_ntt.s: the step's "
                         "blocks hold 2130 for four butterflies, 350 of them per Montgomery product)")
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("ntt_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    rows, clocks = [], []
    try:
        for log_n, n_vec in ROWS:
            n = 1 << log_n
            nbytes = 32 * n * n_vec
            raw = np.random.default_rng(7).integers(0, 256, size=nbytes, dtype=np.uint8)
            raw[31::32] &= 0x1F                                              # every record < 2^253 < r
            scalars = raw.tobytes()
            d_in, d_out = cfg.alloc(nbytes), cfg.alloc(nbytes)
            cfg.to_device(d_in, scalars)
            dom = cfg.ntt_domain(pkg.NTT_ROOT_H2C, log_n)
            if not rows:                                                     # pre-warm once, on the first row's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    cfg.ntt_device(dom, d_in, d_out, n_vec=n_vec)
            for _ in range(args.warmup):
                cfg.ntt_device(dom, d_in, d_out, n_vec=n_vec)
            clk = shader_clock_mhz(cfg.device())
            kernel, wall = [], []
            for _ in range(args.iters):
                t0 = time.perf_counter()
                kernel.append(cfg.ntt_device(dom, d_in, d_out, n_vec=n_vec))
                wall.append((time.perf_counter() - t0) * 1e3)
            got = cfg.to_host(d_out, min(nbytes, 1 << 20))
            host = []
            for _ in range(args.host_iters):
                t0 = time.perf_counter()
                ref = pkg.host_ntt(scalars, pkg.NTT_ROOT_H2C, log_n, n_vec=n_vec, threads=16)
                host.append((time.perf_counter() - t0) * 1e3)
            if ref[:len(got)] != got:
                raise SystemExit(f"ntt_bench.py: GPU and host twin differ at log_n={log_n}")
            dom.free()
            cfg.free(d_in)
            cfg.free(d_out)
            passes = max(1, -(-log_n // 10))
            k_ms = statistics.median(kernel)
            mhz = clk or args.nominal_mhz
            hbm_ms = passes * 64.0 * n * n_vec / HBM_BYTES_PER_S * 1e3
            issue_ms = args.valu_per_butterfly * (n / 2) * log_n * n_vec / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
            clocks.append(clk)
            rows.append({
                "log_n": log_n, "n_vec": n_vec, "passes": passes,
                "kernel_ms": round(k_ms, 4), "wall_ms": round(statistics.median(wall), 4),
                "host_ntt_16_threads_ms": round(statistics.median(host), 2),
                "speedup_over_host": round(statistics.median(host) / statistics.median(wall), 1),
                "sclk_mhz": clk,
                "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
                "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
                "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
            })
            print(json.dumps(rows[-1]), flush=True)
    finally:
        cfg.close()
    result = {
        "tool": "tools/ntt_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_butterfly": args.valu_per_butterfly,
        "setting": "device-resident, MONT_LE, FORWARD, no shift, out of place; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
