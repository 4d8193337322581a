#!/usr/bin/env python3
"""Time the term-list sumcheck calls over Fr on one GPU against the kernels they generalise and the calls they replace
(DESIGN.md section 8.17).

Device-resident buffers, MSM_AMD_SCALAR_MONT_LE, the protocol of tools/mle_bench.py: the clock pre-warmed, each figure the
median of --iters timed calls after --warmup more, the parent's kernels timed in the same run.
  generic    msm_amd_fr_sumcheck_round_terms (device memory) on the lists that spell PRODUCT of two tables and EQ_AB_C, next to
             msm_amd_fr_sumcheck_round_device on the same buffer, kernel ms, at 2^20 and 2^24 (no gate: the ratio is the result)
  product    the round of HyperPlonk's vanilla gate under eq (nine tables, d = 4) at 2^24: kernel ms over the products per
             pair the kernel performs, against the EQ_AB_C kernel over its 8, with the 1.25x margin of DESIGN.md section 8.7,
             and the HBM and issue bounds of the row
  step       msm_amd_fr_sumcheck_step_terms (device memory) against msm_amd_fr_mle_bind_device(1) + the round at n / 2, call
             ms, at 2^16, 2^20, 2^24, both orders, out of place, for three lists: the step must not be slower than the pair
             (the pair is timed as the two calls in turn, so that neither finds its tables in a cache the other left cold)
  sumcheck   a whole sumcheck of m = 20 variables of the gate, in place (HIGH): round_terms, m - 1 steps and the last bind
             against m rounds and m binds
Writes profiles/sumcheck_terms_bench.json.

  python tools/sumcheck_terms_bench.py [--iters 20] [--warmup 3] [--out profiles/sumcheck_terms_bench.json]
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

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
ONE, MINUS_ONE = (MONT.to_bytes(32, "little"), ((R - 1) * MONT % R).to_bytes(32, "little"))     # MONT_LE records
PRODUCT_2 = ([(ONE, [0, 1])], None)
EQ_AB_C = ([(ONE, [1, 2]), (MINUS_ONE, [3])], 0)
# eq (q_L w_1 + q_R w_2 + q_M w_1 w_2 - q_O w_3 + q_C): tables eq, q_L, q_R, q_M, q_O, q_C, w_1, w_2, w_3
VANILLA = ([(ONE, [1, 6]), (ONE, [2, 7]), (ONE, [3, 6, 7]), (MINUS_ONE, [4, 8]), (ONE, [5])], 0)


def counted(form, n_vec):
    """(products, record loads, additions, HBM bytes) per pair of the round kernel's order (fr_mle.hip.h, FrTermSums): passes of
    W values; per pass every factor is loaded (two records), differenced and advanced, a coefficient other than 1 and r - 1 costs
    two products, the outer factor one product per value"""
    terms, outer = form
    values = max(len(f) for _, f in terms) + (outer is not None) + 1
    w = values if values <= 4 else 3 if values <= 7 else 2
    passes = [(t0, min(w, values - t0)) for t0 in range(0, values, w)]
    products = loads = adds = 0
    for t0, width in passes:
        uses = sum(len(f) for _, f in terms) + (outer is not None)
        loads += 2 * uses
        adds += uses * (1 + t0 + width - 1) + len(terms) * width + width
        products += sum((len(f) - 1) * width + (0 if c in (ONE, MINUS_ONE) else 2) for c, f in terms) + (width if outer is not None else 0)
    return products, loads, adds, 64 * n_vec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prewarm-ms", type=int, default=1500, help="untimed load before the first row (GPU clock ramp)")
    ap.add_argument("--valu-per-product", type=float, default=350.0)
    ap.add_argument("--valu-per-load", type=float, default=120.0)
    ap.add_argument("--valu-per-add", type=float, default=40.0)
    ap.add_argument("--nominal-mhz", type=int, default=2400)
    ap.add_argument("--margin", type=float, default=1.25, help="DESIGN.md section 8.7: the same work in another shape")
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--sumcheck-log", type=int, default=20)
    ap.add_argument("--commit", default=None, help="recorded as it is (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck_terms_bench.json"))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("sumcheck_terms_bench.py: --iters must be >= 20")
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    T = lambda form: pkg.SumcheckTerms(*form)                                                            # noqa: E731
    product_2, eq_ab_c, vanilla = T(PRODUCT_2), T(EQ_AB_C), T(VANILLA)
    HIGH, LOW = pkg.MLE_HIGH, pkg.MLE_LOW
    cfg = pkg.setup_metal_state(0)
    rows = []
    r = table(1, 11)

    def bounds(form, n_vec, pairs, k_ms, mhz):
        prod, loads, adds, hbm_bytes = counted(form, n_vec)
        valu = prod * args.valu_per_product + loads * args.valu_per_load + adds * args.valu_per_add
        hbm_ms = hbm_bytes * pairs / HBM_BYTES_PER_S * 1e3
        issue_ms = valu * pairs / (LANES_PER_CYCLE * mhz * 1e6) * 1e3
        return {"products_per_pair": prod, "loads_per_pair": loads, "additions_per_pair": adds, "valu_per_pair": valu,
                "hbm_bound_ms": round(hbm_ms, 4), "hbm_fraction": round(hbm_ms / k_ms, 3), "issue_bound_ms": round(issue_ms, 4),
                "issue_fraction": round(issue_ms / k_ms, 3), "limiter": "issue" if issue_ms >= hbm_ms else "hbm"}

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    try:
        for log_n in args.logs:
            n = 1 << log_n
            a = table(n)
            d_in, d_out = cfg.alloc(32 * n * 9), cfg.alloc(32 * n * 9)
            for v in range(9):
                cfg.to_device(d_in + 32 * n * v, a)
            if not rows:                                                     # pre-warm once, on the first size's load
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
                    cfg.fr_sumcheck_round_terms_device(d_in, n, vanilla, HIGH, n_vec=9)
            kernel = lambda call: median_ms(lambda: call()[1], args.warmup, args.iters)                  # noqa: E731
            if log_n >= 20:
                ms = {}
                for name, call in (
                        ("round_product_2", lambda: cfg.fr_sumcheck_round_device(d_in, n, pkg.SUMCHECK_PRODUCT, HIGH, n_vec=2)),
                        ("round_terms_product_2", lambda: cfg.fr_sumcheck_round_terms_device(d_in, n, product_2, HIGH, n_vec=2)),
                        ("round_eq_ab_c", lambda: cfg.fr_sumcheck_round_device(d_in, n, pkg.SUMCHECK_EQ_AB_C, HIGH, n_vec=4)),
                        ("round_terms_eq_ab_c", lambda: cfg.fr_sumcheck_round_terms_device(d_in, n, eq_ab_c, HIGH, n_vec=4)),
                        ("round_terms_vanilla", lambda: cfg.fr_sumcheck_round_terms_device(d_in, n, vanilla, HIGH, n_vec=9))):
                    ms[name], wall = kernel(call)
                    emit({"section": "generic", "op": name, "log_n": log_n, "kernel_ms": round(ms[name], 4), "wall_ms": round(wall, 4),
                          "sclk_mhz": shader_clock_mhz(cfg.device())})
                if log_n <= 20 and call()[0] != cfg.fr_sumcheck_round_terms(a * 9, n, vanilla, HIGH, n_vec=9):
                    raise SystemExit("sumcheck_terms_bench.py: device and host-buffer form differ")
                for generic, parent in (("round_terms_product_2", "round_product_2"), ("round_terms_eq_ab_c", "round_eq_ab_c")):
                    emit({"section": "generic", "op": generic + " / " + parent, "log_n": log_n, "ratio": round(ms[generic] / ms[parent], 3),
                          "gate": None})
                if log_n == max(args.logs):
                    mhz = shader_clock_mhz(cfg.device()) or args.nominal_mhz
                    prod = counted(VANILLA, 9)[0]
                    per, parent = ms["round_terms_vanilla"] / prod, ms["round_eq_ab_c"] / 8
                    row = {"section": "product", "op": "round_terms_vanilla", "log_n": log_n, "kernel_ms": round(ms["round_terms_vanilla"], 4),
                           "ms_per_product": round(per, 5), "parent": "round_eq_ab_c", "parent_ms_per_product": round(parent, 5),
                           "ratio": round(per / parent, 3), "ratio_bound": args.margin, "within_bound": bool(per / parent <= args.margin)}
                    row.update(bounds(VANILLA, 9, n // 2, ms["round_terms_vanilla"], mhz))
                    emit(row)
                    emit(dict({"section": "product", "op": "round_eq_ab_c", "log_n": log_n, "kernel_ms": round(ms["round_eq_ab_c"], 4)},
                              **bounds(EQ_AB_C, 4, n // 2, ms["round_eq_ab_c"], mhz)))
            for form_name, terms, k in (("product_2", product_2, 2), ("eq_ab_c", eq_ab_c, 4), ("vanilla", vanilla, 9)):
                for order, name in ((HIGH, "high"), (LOW, "low")):
                    wall = lambda call: median_ms(call, args.warmup, args.iters)[1]                       # noqa: E731
                    step = wall(lambda: cfg.fr_sumcheck_step_terms_device(d_in, n, d_out, r, terms, order, n_vec=k)[1])

                    def pair():              # the two calls in turn, as a prover issues them: neither finds its tables in a cache
                        cfg.fr_mle_bind_device(d_in, n, d_out, r, order, n_vec=k)
                        return cfg.fr_sumcheck_round_terms_device(d_out, n // 2, terms, order, n_vec=k, stride=n)[1]

                    both = wall(pair)
                    emit({"section": "step", "op": "step_terms_%s_%s" % (form_name, name), "log_n": log_n, "step_call_ms": round(step, 4),
                          "pair_call_ms": round(both, 4), "ratio": round(step / both, 3), "not_slower": bool(step <= both)})
            if log_n == args.sumcheck_log:
                point = table(log_n, 12)
                rec = lambda s: point[32 * s:32 * s + 32]                                                # noqa: E731

                def fused():
                    t0, size = time.perf_counter(), n
                    cfg.fr_sumcheck_round_terms_device(d_out, size, vanilla, HIGH, n_vec=9, stride=n)
                    for s in range(log_n - 1):
                        cfg.fr_sumcheck_step_terms_device(d_out, size, d_out, rec(s), vanilla, HIGH, n_vec=9, stride=n)
                        size //= 2
                    cfg.fr_mle_bind_device(d_out, size, d_out, rec(log_n - 1), HIGH, n_vec=9, stride=n)
                    return (time.perf_counter() - t0) * 1e3

                def separate():
                    t0, size = time.perf_counter(), n
                    for s in range(log_n):
                        cfg.fr_sumcheck_round_terms_device(d_out, size, vanilla, HIGH, n_vec=9, stride=n)
                        cfg.fr_mle_bind_device(d_out, size, d_out, rec(s), HIGH, n_vec=9, stride=n)
                        size //= 2
                    return (time.perf_counter() - t0) * 1e3

                one, _ = median_ms(fused, args.warmup, args.iters)
                two, _ = median_ms(separate, args.warmup, args.iters)
                emit({"section": "sumcheck", "op": "vanilla gate, m = %d, HIGH in place" % log_n, "calls_fused": log_n + 1,
                      "calls_separate": 2 * log_n, "fused_ms": round(one, 4), "separate_ms": round(two, 4), "ratio": round(one / two, 3)})
            cfg.free(d_in)
            cfg.free(d_out)
    finally:
        cfg.close()
    result = {
        "tool": "tools/sumcheck_terms_bench.py", "box": socket.gethostname(), "commit": args.commit or commit(),
        "nominal_mhz": args.nominal_mhz, "iters": args.iters, "warmup": args.warmup, "prewarm_ms": args.prewarm_ms,
        "valu_per_product": args.valu_per_product, "valu_per_load": args.valu_per_load, "valu_per_add": args.valu_per_add,
        "setting": "device-resident, MONT_LE, nine tables of the same records; median of the timed calls; the contents of the "
                   "tables do not enter the time, so the whole sumcheck runs on what the previous one left",
        "rows": rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
