"""Pairing throughput on one MI355X: tools/pairing_bench.py [--out profiles/pairing_bench.json] [--max-log 16]

Rows: pairs/s of msm_amd_pairing_product for one product (n_groups = 1, group_size 2^10 .. 2^max-log) and for independent
groups (group_size 1 and 4, n_groups 2^8 .. 2^(max-log - 2)), device-resident (kernel_ms and wall time of the blocking
call) and from host buffers, with the host twin at 16 threads beside them.  Each row also holds the kernel time of its two
stages, taken at the stage tap and not by subtraction: miller_fold_ms (the same call with MSM_AMD_PAIRING_MILLER_ONLY: the
Miller kernel, the fold levels and the conversion of one record per group) and final_ms (msm_amd_final_exponentiation_device
on the group count).  Three A/Bs decide the shipped plan:
  f in LDS         the running f of the Miller kernel in private memory against LDS, word-major, at 2^14 pairs
  pairs per lane   1, 2, 4 at 2^14 pairs (one group, and 2^12 groups of 4), alternated --rounds times
  final exponentiation   the device kernel against the host twin at 16 threads over n = 16 .. 4096 records: the smallest
                         n from which the device wins is the crossover behind MSM_AMD_PAIRING_DEVICE_FINAL_FROM
Method (measuring-on-mi355x): an untimed pre-warm so the clock has ramped, warm-up calls per row, the median of the
repeats, A/B arms alternated in one process, the shader clock read while the load runs.  Inputs: a short progression of
points repeated to length (a pairing costs the same for every valid pair)."""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ntt_bench import commit, shader_clock_mhz  # noqa: E402

GT = 384


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        r = fn()
        out.append(((time.perf_counter() - t) * 1e3, r))
    wall = statistics.median(w for w, _ in out)
    ks = [r for _, r in out if isinstance(r, float)]
    return wall, (statistics.median(ks) if ks else None)


def knobs(ppl=None, final_from=None, lds=None):
    for name, v in (("MSM_AMD_PAIRING_PAIRS_PER_LANE", ppl), ("MSM_AMD_PAIRING_DEVICE_FINAL_FROM", final_from),
                    ("MSM_AMD_PAIRING_F_IN_LDS", lds)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def shipped(m):
    """the defaults of the library this run used, asked of the library: the planner with nothing set, the first group
    count whose plan finishes on the device, and the kernel's default home of f (a constant of launch_pairing.h)"""
    lo, hi = 0, 1 << 31
    while lo + 1 < hi:                                   # final_on_device is monotone in n_groups
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if m.pairing_plan(mid, 1)["final_on_device"] else (mid, hi)
    hdr = open(os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc", "launch_pairing.h")).read()
    lds = re.search(r"constexpr bool kPairingFInLds = (true|false);", hdr).group(1) == "true"
    return {"device_final_from": hi, "pairs_per_lane": sorted({m.pairing_plan(1, 1 << lg)["pairs_per_lane"] for lg in range(0, 31)}),
            "f_in_lds": lds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_bench.json"))
    ap.add_argument("--max-log", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-max-log", type=int, default=12, help="largest size the host twin is timed at")
    args = ap.parse_args()
    m = importlib.import_module("metal-msm-gpu-acceleration_amd")
    import mul_ref as mr
    import g2_ref as g2
    from oracle import bn254_ref as o
    cfg = m.setup_metal_state(0)
    nmax = 1 << args.max_log
    base = 256
    sc = [3 + 7 * i for i in range(base)]
    g1 = m.host_mul_points(mr.scalars_bytes(sc, 0), mr.base_record(1, 0, o.GEN), base, mr.ONE)
    q = m.host_mul_points(mr.scalars_bytes(sc[::-1], 0), mr.base_record(2, 0, g2.GEN2), base, mr.ONE, g2=True)
    g1, q = g1 * (nmax // base), q * (nmax // base)
    d1, d2 = cfg.alloc(len(g1)), cfg.alloc(len(q))
    cfg.to_device(d1, g1)
    cfg.to_device(d2, q)
    d_out, d_one = cfg.alloc(nmax * GT), cfg.alloc(nmax)
    knobs()
    t_end = time.perf_counter() + 1.5                       # pre-warm: the clock ramps under load
    while time.perf_counter() < t_end:
        cfg.pairing_product_device(d1, d2, 1 << 10, 1, d_out, d_one)
    rows, clocks = [], []

    def row(n_groups, size, label):
        n = n_groups * size
        knobs(final_from=0)
        wall_d, kern = timed(lambda: cfg.pairing_product_device(d1, d2, n_groups, size, d_out, d_one), args.warmup, args.iters)
        _, mil = timed(lambda: cfg.pairing_product_device(d1, d2, n_groups, size, d_out, None, flags=m.PAIRING_MILLER_ONLY),
                       args.warmup, args.iters)
        _, fin = timed(lambda: cfg.final_exponentiation_device(d_out, n_groups, d_out, d_one), args.warmup, args.iters)
        clk = shader_clock_mhz(cfg.device()) if hasattr(cfg, "device") else None
        clocks.append(clk)
        knobs()
        wall_h, _ = timed(lambda: cfg.pairing_product(g1[:64 * n], q[:128 * n], n_groups, size) and None, args.warmup, args.iters)
        host = None
        if n <= 1 << args.host_max_log:
            host, _ = timed(lambda: m.host_pairing_product(g1[:64 * n], q[:128 * n], n_groups, size, threads=16) and None, 0, 1)
        plan = m.pairing_plan(n_groups, size)
        r = {"shape": label, "n_groups": n_groups, "group_size": size, "pairs": n, "kernel_ms": kern, "miller_fold_ms": mil,
             "final_ms": fin, "device_wall_ms": wall_d,
             "host_buffers_wall_ms": wall_h, "host_twin_16_threads_ms": host, "pairs_per_s_device": n / (kern * 1e-3),
             "pairs_per_s_host_buffers": n / (wall_h * 1e-3), "pairs_per_s_host_twin": (n / (host * 1e-3)) if host else None,
             "plan": plan, "sclk_mhz": clk}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for lg in range(10, args.max_log + 1, 2):
        row(1, 1 << lg, "one product")
    for size in (1, 4):
        for lg in range(8, args.max_log - 1, 2):
            if (1 << lg) * size <= nmax:
                row(1 << lg, size, "independent groups of %d" % size)

    # A/B 0: where the running f lives, at 2^14 pairs: the whole call and the Miller stage alone
    ab_lds = []
    for n_groups, size in ((1, 1 << 14), (1 << 12, 4)):
        arms = {0: {"kernel_ms": [], "miller_fold_ms": []}, 1: {"kernel_ms": [], "miller_fold_ms": []}}
        for _ in range(args.rounds):
            for lds in (0, 1):
                knobs(1, 0, lds)
                _, kern = timed(lambda: cfg.pairing_product_device(d1, d2, n_groups, size, d_out, d_one), 0, 1)
                _, mil = timed(lambda: cfg.pairing_product_device(d1, d2, n_groups, size, d_out, None, flags=m.PAIRING_MILLER_ONLY), 0, 1)
                arms[lds]["kernel_ms"].append(kern)
                arms[lds]["miller_fold_ms"].append(mil)
        ab_lds.append({"n_groups": n_groups, "group_size": size, "private": arms[0], "lds": arms[1],
                       "median_miller_fold_ms": {"private": statistics.median(arms[0]["miller_fold_ms"]),
                                                 "lds": statistics.median(arms[1]["miller_fold_ms"])}})
        print(json.dumps(ab_lds[-1]), flush=True)

    # A/B 1: pairs per lane at 2^14 pairs
    ab_ppl = []
    for n_groups, size in ((1, 1 << 14), (1 << 12, 4)):
        arms = {1: [], 2: [], 4: []}
        for _ in range(args.rounds):
            for ppl in (1, 2, 4):
                knobs(ppl, 0)
                _, kern = timed(lambda: cfg.pairing_product_device(d1, d2, n_groups, size, d_out, None, flags=m.PAIRING_MILLER_ONLY), 0, 1)
                arms[ppl].append(kern)
        ab_ppl.append({"n_groups": n_groups, "group_size": size,
                       "miller_fold_ms": {str(k): v for k, v in arms.items()},
                       "median_ms": {str(k): statistics.median(v) for k, v in arms.items()}})
        print(json.dumps(ab_ppl[-1]), flush=True)

    # A/B 2: where the final exponentiation runs
    knobs()
    recs, _ = m.host_pairing_product(g1[:64 * 4096], q[:128 * 4096], 4096, 1, flags=m.PAIRING_MILLER_ONLY)
    d_in = cfg.alloc(len(recs))
    cfg.to_device(d_in, recs)
    ab_final, crossover = [], None
    for n in (16, 64, 256, 1024, 4096):
        dev, hst = [], []
        for _ in range(args.rounds):
            t = time.perf_counter()
            cfg.final_exponentiation_device(d_in, n, d_out, d_one)
            dev.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            m.host_final_exponentiation(recs[:n * GT], n, threads=16)
            hst.append((time.perf_counter() - t) * 1e3)
        e = {"n": n, "device_wall_ms": dev, "host_16_threads_ms": hst, "device_median_ms": statistics.median(dev),
             "host_median_ms": statistics.median(hst)}
        if crossover is None and e["device_median_ms"] < e["host_median_ms"]:
            crossover = n
        ab_final.append(e)
        print(json.dumps(e), flush=True)
    doc = {"tool": "tools/pairing_bench.py", "commit": commit(), "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
           "host_cpus": os.cpu_count(), "sclk_mhz": clocks, "rows": rows, "ab_f_in_lds": ab_lds, "ab_pairs_per_lane": ab_ppl,
           "ab_final_exponentiation": ab_final, "final_exponentiation_crossover_n": crossover, "shipped": shipped(m)}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for d in (d1, d2, d_out, d_one, d_in):
        cfg.free(d)
    cfg.close()


if __name__ == "__main__":
    main()
