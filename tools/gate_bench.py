#!/usr/bin/env python3
"""Time msm_amd_fr_gate_eval on one GPU against what a caller has without it.

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, the protocol of tools/mle_bench.py: the clock pre-warmed, each figure the
median of --iters timed calls after --warmup more; the fused call and the chain it replaces alternate inside one timed loop, so
that both see the same clock and the same neighbours.
  gate     the vanilla PLONK gate q_L a + q_R b + q_M a b - q_O c + q_C without rotations over eight columns: kernel ms of the one
           call against the summed kernel ms of the equivalent chain of msm_amd_fr_map_device calls, four MUL and four ADD / SUB
           (a (q_L + q_M b) + q_R b - q_O c + q_C).  The fused kernel must not take longer than the chain: the chain moves 8 x 96
           bytes per row, the call 8 reads and 1 write of 32.  No further margin.
  shape    the same gate with c one row on, ACCUMULATE and a scale of period 4 (what the last call of an evaluate_h chain does):
           kernel ms, no gate
  read     kernel ms per record read (the ten factors of the gate) over that of the FR_MUL kernel (two) at the same n: the
           yardstick of sections 8.7 and 8.9, no gate
  bytes    the 8 columns and the output once over the HBM roofline
  twin     msm_amd_host_fr_gate_eval at 16 threads, up to --host-max-log
Writes profiles/gate_bench.json.

  python tools/gate_bench.py [--iters 20] [--warmup 3] [--out profiles/gate_bench.json]
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
from mle_bench import median_ms, table  # noqa: E402
from ntt_bench import HBM_BYTES_PER_S, commit, shader_clock_mhz  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
ONE, MINUS_ONE = (MONT.to_bytes(32, "little"), ((R - 1) * MONT % R).to_bytes(32, "little"))     # MONT_LE records
QL, QR, QM, QO, QC, A, B, C = range(8)


def vanilla(c_rot=0):
    return [(ONE, [QL, A]), (ONE, [QR, B]), (ONE, [QM, A, B]), (MINUS_ONE, [QO, (C, c_rot)]), (ONE, [QC])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--host-max-log", type=int, default=20, help="the host twin runs up to this size")
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("gate_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    plain, shaped = pkg.GateTerms(vanilla()), pkg.GateTerms(vanilla(1))
    cfg = pkg.setup_metal_state(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    try:
        for log_n in args.logs:
            n = 1 << log_n
            d_in, d_out, d_t, d_u = cfg.alloc(32 * n * 8), cfg.alloc(32 * n), cfg.alloc(32 * n), cfg.alloc(32 * n)
            cols = [table(n, 20 + v) for v in range(8)]
            for v in range(8):
                cfg.to_device(d_in + 32 * n * v, cols[v])
            col = lambda v: d_in + 32 * n * v                                                            # noqa: E731
            fused = lambda: cfg.fr_gate_eval(d_in, plain, n, 8, out=d_out, mem=pkg.MEM_DEVICE)[1]      # noqa: E731

            def chain():
                m = lambda op, a, b, out: cfg.fr_map_device(op, a, b, None, n, out)                     # noqa: E731
                return (m(pkg.FR_MUL, col(QM), col(B), d_t) + m(pkg.FR_ADD, d_t, col(QL), d_t) + m(pkg.FR_MUL, d_t, col(A), d_t) +
                        m(pkg.FR_MUL, col(QR), col(B), d_u) + m(pkg.FR_ADD, d_t, d_u, d_t) + m(pkg.FR_MUL, col(QO), col(C), d_u) +
                        m(pkg.FR_SUB, d_t, d_u, d_t) + m(pkg.FR_ADD, d_t, col(QC), d_t))

            if not rows:                                                     # pre-warm once, on the first size's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    fused()
            for _ in range(args.warmup):
                fused(), chain()
            if cfg.to_host(d_out, 32 * n) != cfg.to_host(d_t, 32 * n):
                raise SystemExit("gate_bench.py: the call and the chain of maps differ")
            k_fused, k_chain, w_fused, w_chain = [], [], [], []
            for _ in range(args.iters):                                      # alternating: the same clock for both
                t0 = time.perf_counter()
                k_fused.append(fused())
                t1 = time.perf_counter()
                k_chain.append(chain())
                t2 = time.perf_counter()
                w_fused.append((t1 - t0) * 1e3), w_chain.append((t2 - t1) * 1e3)
            f_ms, c_ms = statistics.median(k_fused), statistics.median(k_chain)
            hbm_ms = 9 * 32 * n / HBM_BYTES_PER_S * 1e3
            emit({"section": "gate", "op": "vanilla gate, no rotations", "log_n": log_n, "kernel_ms": round(f_ms, 4),
                  "call_ms": round(statistics.median(w_fused), 4), "chain_kernel_ms": round(c_ms, 4),
                  "chain_call_ms": round(statistics.median(w_chain), 4), "ratio": round(f_ms / c_ms, 3), "ratio_bound": 1.0,
                  "within_bound": bool(f_ms <= c_ms), "kernel_ms_min_max": [round(min(k_fused), 4), round(max(k_fused), 4)],
                  "chain_kernel_ms_min_max": [round(min(k_chain), 4), round(max(k_chain), 4)],
                  "products_per_row": pkg.test_fr_gate_plan(plain, n, 8)["products"], "reads_per_row": 10,
                  "hbm_bytes": 9 * 32 * n, "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / f_ms, 3),
                  "sclk_mhz": shader_clock_mhz(cfg.device())})
            mul_ms, _ = median_ms(lambda: cfg.fr_map_device(pkg.FR_MUL, col(A), col(B), None, n, d_u), args.warmup, args.iters)
            emit({"section": "read", "op": "gate / FR_MUL, kernel ms per record read", "log_n": log_n, "fr_mul_kernel_ms": round(mul_ms, 4),
                  "gate_ms_per_read": round(f_ms / 10, 5), "fr_mul_ms_per_read": round(mul_ms / 2, 5),
                  "ratio": round((f_ms / 10) / (mul_ms / 2), 3), "gate": None})
            scale = table(4, 5)
            s_ms, s_wall = median_ms(lambda: cfg.fr_gate_eval(d_in, shaped, n, 8, rot_step=4, flags=pkg.GATE_ACCUMULATE, k_acc=ONE,
                                                              scale=scale, out=d_out, mem=pkg.MEM_DEVICE)[1], args.warmup, args.iters)
            emit({"section": "shape", "op": "c at rotation +1, rot_step 4, ACCUMULATE, scale of period 4", "log_n": log_n,
                  "kernel_ms": round(s_ms, 4), "call_ms": round(s_wall, 4),
                  "products_per_row": pkg.test_fr_gate_plan(shaped, n, 8, 4, pkg.GATE_ACCUMULATE, 4)["products"], "gate": None})
            if log_n <= args.host_max_log:
                data = b"".join(cols)
                t0 = time.perf_counter()
                twin = pkg.host_fr_gate_eval(data, plain, n, 8, threads=16)
                host_ms = (time.perf_counter() - t0) * 1e3
                if twin != cfg.to_host(d_t, 32 * n):
                    raise SystemExit("gate_bench.py: the twin and the device differ")
                emit({"section": "twin", "op": "msm_amd_host_fr_gate_eval, 16 threads", "log_n": log_n, "host_ms": round(host_ms, 3),
                      "device_call_ms": round(statistics.median(w_fused), 4)})
            for d in (d_in, d_out, d_t, d_u):
                cfg.free(d)
    finally:
        cfg.close()
    result = {
        "tool": "tools/gate_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(), "iters": args.iters,
        "warmup": args.warmup, "prewarm_ms": args.prewarm_ms, "hbm_bytes_per_s": HBM_BYTES_PER_S,
        "setting": "device-resident, MONT_LE, eight columns of random records; the fused call and the chain of eight map calls "
                   "alternate in one timed loop; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
