#!/usr/bin/env python3
"""Time the Poseidon calls over Fr on one GPU against their host twins and against the kernel they are held to (DESIGN.md
section 8.11).

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, circomlib's constants: the hash for t = 3 and t = 5 at 2^16, 2^20 and 2^22
digests, the binary tree over 2^20 leaves, its paths for 2^10 indices -- and, same run, same build, the yardstick: the
eq table of section 8.9 at 2^24 outputs (4.25 products per output).  The clock is pre-warmed as in tools/fr_bench.py; each row is
the median of --iters timed calls after --warmup more: kernel_ms as the call reports it and the wall time of the blocking
call.  The baseline is the host twin at 16 threads on the same box at 2^20 (its bytes must equal the device's).  Bounds per
row, per element (a digest, a node of the tree, an output of the eq table):
  hbm    bytes read + written x elements over 8 TB/s
  issue  VALU per element x elements over 256 CUs x 4 SIMDs x 64 lanes / 4 cycles at the clock the run reports, VALU =
         products x 350 + operand loads x 120 + additions x 40 (the weights of tools/fr_bench.py); a textbook permutation
         counts 3 (R_F t + R_P) + (R_F + R_P) t^2 products and (R_F + R_P) t^2 additions
The gate: kernel time per counted product of the t = 3 hash at 2^22 over that of the eq table at 2^24, at most 1.25.
--sweep LOG ..: the tree once more on a fresh ctx per MSM_AMD_POSEIDON_TOP_LOG, written to --sweep-out as text.
Writes profiles/poseidon_bench.json and the rows of the DESIGN table (--table-out).

  python tools/poseidon_bench.py [--iters 20] [--warmup 3] [--sweep 6 8 10] [--out profiles/poseidon_bench.json]
"""
import argparse
import importlib
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mle_bench import median_ms, table  # noqa: E402
from ntt_bench import HBM_BYTES_PER_S, LANES_PER_CYCLE, commit, shader_clock_mhz  # noqa: E402

R_F = 8
HASH_LOGS = (16, 20, 22)
TREE_LOG = 20
YARD_LOG = 24
GATE = 1.25


def products(t, r_p):
    return 3 * (R_F * t + r_p) + (R_F + r_p) * t * t


def additions(t, r_p):
    return (R_F + r_p) * t * t


def sweep(pkg, args):
    """the binary tree at every top log of the sweep, a fresh ctx each"""
    lines = ["# tools/poseidon_bench.py --sweep: kernel_ms of msm_amd_poseidon_merkle_build_device, t = 3, MONT_LE; median of %d "
             "after %d" % (args.iters, args.warmup), "# top_log  log_leaves  launches  tail_levels  kernel_ms"]
    best = {}
    for log_n in (12, 16, TREE_LOG):
        n = 1 << log_n
        leaves = table(n)
        for top_log in args.sweep:
            os.environ["MSM_AMD_POSEIDON_TOP_LOG"] = str(top_log)
            cfg = pkg.setup_metal_state(0)
            try:
                h = cfg.poseidon_params(3)
                d_leaves, d_tree = cfg.alloc(32 * n), cfg.alloc(32 * n)
                cfg.to_device(d_leaves, leaves)
                k_ms, _ = median_ms(lambda: cfg.poseidon_merkle_build_device(h, d_leaves, n, d_tree, want_root=False)[1],
                                    args.warmup, args.iters)
                plan = pkg.test_poseidon_plan(3, n, top_log)
                lines.append("%-9d %-11d %-9d %-12d %.4f" % (top_log, log_n, plan["launches"], plan["tail_levels"], k_ms))
                best.setdefault(log_n, []).append((k_ms, top_log))
                print(lines[-1], flush=True)
                cfg.free(d_leaves)
                cfg.free(d_tree)
            finally:
                cfg.close()
    os.environ.pop("MSM_AMD_POSEIDON_TOP_LOG", None)
    for log_n, got in sorted(best.items()):
        lines.append("# fastest at 2^%d leaves: top_log %d" % (log_n, min(got)[1]))
    os.makedirs(os.path.dirname(args.sweep_out), exist_ok=True)
    with open(args.sweep_out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--host-log", type=int, default=20, help="the host twins run at this size")
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--sweep", type=int, nargs="*", default=[], help="top logs of the tree to sweep first")
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "poseidon_ab.txt"))
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_bench.json"))
    ap.add_argument("--table-out", default=None, help="the rows of the DESIGN table, as markdown")
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("poseidon_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    if args.sweep:
        sweep(pkg, args)
    cfg = pkg.setup_metal_state(0)
    rows, clocks = [], []

    def row(op, log_n, elements, counted, call, host=None, check=None):
        """counted: (products, loads, additions, HBM bytes) per element; host(): the twin's bytes; check(): the device's"""
        k_ms, w_ms = median_ms(call, args.warmup, args.iters)
        clk = shader_clock_mhz(cfg.device())
        h_ms = None
        if host is not None:
            got = check()
            t0 = time.perf_counter()
            ref = host()
            h_ms = (time.perf_counter() - t0) * 1e3
            if ref[:len(got)] != got:
                raise SystemExit(f"poseidon_bench.py: GPU and host twin differ: {op} at log_n={log_n}")
        mhz = clk or args.nominal_mhz
        prod, loads, adds, hbm_bytes = counted
        valu = prod * args.valu_per_product + loads * args.valu_per_load + adds * args.valu_per_add
        hbm_ms = hbm_bytes * elements / HBM_BYTES_PER_S * 1e3
        issue_ms = valu * elements / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
        clocks.append(clk)
        rows.append({
            "op": op, "log_n": log_n, "elements": elements, "kernel_ms": round(k_ms, 4), "wall_ms": round(w_ms, 4),
            "host_twin_16_threads_ms": None if h_ms is None else round(h_ms, 2),
            "speedup_over_host": None if h_ms is None else round(h_ms / w_ms, 1),
            "sclk_mhz": clk, "products_per_element": prod, "additions_per_element": adds, "valu_per_element": valu,
            "ns_per_product": round(k_ms * 1e6 / (elements * prod), 6) if prod else None,
            "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3),
            "issue_bound_ms": round(issue_ms, 4), "issue_fraction": round(issue_ms / k_ms, 3),
            "limiter": "issue" if issue_ms >= hbm_ms else "hbm",
        })
        print(json.dumps(rows[-1]), flush=True)
        return rows[-1]

    try:
        point = table(YARD_LOG, 11)
        d_eq = cfg.alloc(32 << YARD_LOG)
        eq_call = lambda: cfg.fr_eq_table_device(d_eq, point, pkg.MLE_HIGH)   # noqa: E731
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
            eq_call()
        yard = row("eq_table (yardstick)", YARD_LOG, 1 << YARD_LOG, ((YARD_LOG + 10) / 8.0, 0, 0, 32), eq_call)
        cfg.free(d_eq)
        for t in (3, 5):
            r_p = pkg.POSEIDON_R_P[t]
            shape = (t, R_F, r_p) + pkg.poseidon_constants(t)
            h = cfg.poseidon_params(t)
            counted = (products(t, r_p), t - 1, additions(t, r_p), 32 * t)
            for log_n in HASH_LOGS:
                n = 1 << log_n
                data = table(n * (t - 1))
                d_in, d_out = cfg.alloc(len(data)), cfg.alloc(32 * n)
                cfg.to_device(d_in, data)
                at_host = log_n == args.host_log
                got = row("hash t=%d" % t, log_n, n, counted, lambda: cfg.poseidon_hash_device(h, d_in, n, d_out),
                          (lambda: pkg.host_poseidon_hash(*shape, data, n, threads=16)) if at_host else None,
                          lambda: cfg.to_host(d_out, 32 * n))
                if t == 3 and log_n == HASH_LOGS[-1]:
                    got["held_to"] = yard["op"]
                    got["ratio_per_product"] = round(got["ns_per_product"] / yard["ns_per_product"], 3)
                    got["ratio_bound"] = GATE
                    got["within_bound"] = bool(got["ratio_per_product"] <= GATE)
                    print(json.dumps(got), flush=True)
                cfg.free(d_in)
                cfg.free(d_out)
            if t == 3:
                n = 1 << TREE_LOG
                leaves = table(n)
                d_leaves, d_tree = cfg.alloc(32 * n), cfg.alloc(32 * n)
                cfg.to_device(d_leaves, leaves)
                tree = {}
                row("merkle_build t=3", TREE_LOG, n - 1, counted,
                    lambda: cfg.poseidon_merkle_build_device(h, d_leaves, n, d_tree, want_root=False)[1],
                    lambda: tree.setdefault("host", pkg.host_poseidon_merkle_build(*shape, leaves, n, threads=16))[0],
                    lambda: cfg.to_host(d_tree, 32 * (n - 1)))
                idx = [(k * 2654435761) % n for k in range(1 << 10)]
                d_paths = cfg.alloc(32 * len(idx) * TREE_LOG)
                row("merkle_paths t=3, 2^10 indices", TREE_LOG, len(idx) * TREE_LOG, (0, 1, 0, 64),
                    lambda: cfg.poseidon_merkle_paths_device(h, d_leaves, n, d_tree, idx, d_paths),
                    lambda: pkg.host_poseidon_merkle_paths(3, leaves, n, tree["host"][0], idx, threads=16),
                    lambda: cfg.to_host(d_paths, 32 * len(idx) * TREE_LOG))
                for d in (d_leaves, d_tree, d_paths):
                    cfg.free(d)
            h.free()
    finally:
        cfg.close()
    result = {
        "tool": "tools/poseidon_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "sclk_mhz": clocks, "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup,
        "prewarm_ms": args.prewarm_ms, "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load,
        "valu_per_add": args.valu_per_add, "top_log": int(os.environ.get("MSM_AMD_POSEIDON_TOP_LOG", "-1")),
        "setting": "device-resident, MONT_LE, out of place, circomlib constants, tag 0; median of the timed calls",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if args.table_out:
        lines = ["| call | n | kernel ms | call ms | host ms | call vs host | sclk MHz | products / element | ns / product | "
                 "HBM bound ms (share) | issue bound ms (share) | ratio (bound) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            host = "—" if r["host_twin_16_threads_ms"] is None else "%.1f" % r["host_twin_16_threads_ms"]
            speed = "—" if r["speedup_over_host"] is None else "%.0f×" % r["speedup_over_host"]
            ratio = "—" if "ratio_per_product" not in r else "%.2f (≤ %.2f: %s)" % (
                r["ratio_per_product"], r["ratio_bound"], "met" if r["within_bound"] else "MISSED")
            per = "—" if r["ns_per_product"] is None else "%.5f" % r["ns_per_product"]
            lines.append("| `%s` | 2^%d | %.4f | %.4f | %s | %s | %s | %.2f | %s | %.4f (%.0f %%) | %.4f (%.0f %%) | %s |" % (
                r["op"], r["log_n"], r["kernel_ms"], r["wall_ms"], host, speed, r["sclk_mhz"], r["products_per_element"],
                per, r["hbm_bound_ms"], 100 * r["hbm_fraction"], r["issue_bound_ms"], 100 * r["issue_fraction"], ratio))
        with open(args.table_out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
