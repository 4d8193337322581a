#!/usr/bin/env python3
"""Time the sort of Fr records by canonical value on one GPU.

msm_amd_fr_sort, MSM_AMD_SCALAR_CANON_LE, one column of 2^16, 2^20 and 2^22 records, both outputs, on three columns:
full-width random values (all 32 digit passes), values below 2^16 (2 passes) and an all-equal column (none), in both `mem`
forms.  Per case: kernel_ms as the call reports it (the two spans of kernels between events, without the host's read of the
digit mask between them) and the wall time of the blocking call (device form: the kernels, the bounded wait for the mask and
the launches; host form: also the upload of the column and the download of the records and the permutation), each the
median of --iters calls after --warmup more, the clock pre-warmed.  Beside them the host twin at 16 threads on the same box,
whose bytes must equal the device's, and the bytes the passes must move against 8 TB/s.
At the largest size also msm_amd_fr_lookup_permute_as on device buffers over a sorted handle, n = n_rows, both outputs:
MSM_AMD_PERMUTE_HALO2 against MSM_AMD_PERMUTE_ROWS, alternated call by call, and msm_amd_fr_lookup_build_sorted.
Nothing here was alternated against another form of the sort: there is one.  Writes profiles/fr_sort_bench.json.

  python tools/fr_sort_bench.py [--logs 16 20 22] [--iters 10] [--warmup 2] [--out profiles/fr_sort_bench.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ntt_bench import HBM_BYTES_PER_S, commit, shader_clock_mhz  # noqa: E402

DISTRIBUTIONS = ("full_width", "below_2_16", "all_equal")
MASKS = {"full_width": 0xFFFFFFFF, "below_2_16": 0x3, "all_equal": 0}


def column(rng, n, dist):
    """n CANON_LE records"""
    raw = np.zeros((n, 32), dtype=np.uint8)
    if dist == "full_width":
        raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        raw[:, 31] &= 0x1F                                           # every residue < 2^253 < r
    elif dist == "below_2_16":
        raw[:, :2] = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)
    else:
        raw[:, 0] = 7
    return raw.tobytes()


def must_move(n, mask):
    """bytes the kernels of one column must move: the keys pass (32 in, 32 out), per gathered word 4 + 8 + 8, per pass two
    reads and one write of the 8-byte pairs, the final gather (8 + 32 in, 32 + 4 out)"""
    words = sum(1 for w in range(8) if (mask >> (4 * w)) & 0xF)
    passes = bin(mask).count("1")
    return n * (64 + 20 * words + 24 * passes + 76)


def median_call(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    got = [fn() for _ in range(iters)]
    return [statistics.median(g[k] for g in got) for k in range(len(got[0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prewarm-ms", type=int, default=1500)
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--commit", default=None, help="the commit the library was built from, for a run outside a git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_sort_bench.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    layout = pkg.SCALAR_CANON_LE                                     # the columns are built as residues
    rows, clocks, permute_rows = [], [], []
    try:
        big = 1 << max(args.logs)
        d_in, d_out, d_perm = cfg.alloc(32 * big), cfg.alloc(32 * big), cfg.alloc(4 * big)
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.prewarm_ms:
            cfg.fr_shift_device(d_in, big, d_in, bytes(32))
        for log_n in args.logs:
            n = 1 << log_n
            for dist in DISTRIBUTIONS:
                data = column(np.random.default_rng(100 * log_n + DISTRIBUTIONS.index(dist)), n, dist)
                mask = MASKS[dist]
                t0 = time.perf_counter()
                twin_out, twin_perm = pkg.host_fr_sort(data, layout, threads=16)
                twin_ms = (time.perf_counter() - t0) * 1e3
                out, perm = ctypes.create_string_buffer(32 * n), (ctypes.c_uint32 * n)()

                def host_call():
                    t0 = time.perf_counter()
                    ms = cfg.fr_sort(data, layout, 1, pkg.MEM_HOST, n=n, out=out, perm_out=perm)[2]
                    return (time.perf_counter() - t0) * 1e3, ms

                def device_call():
                    t0 = time.perf_counter()
                    ms = cfg.fr_sort(d_in, layout, 1, pkg.MEM_DEVICE, n=n, out=d_out, perm_out=d_perm)[2]
                    return (time.perf_counter() - t0) * 1e3, ms
                cfg.to_device(d_in, data)
                host_wall, host_kernel = median_call(host_call, args.warmup, args.iters)
                dev_wall, dev_kernel = median_call(device_call, args.warmup, args.iters)
                if out.raw != twin_out or list(perm) != twin_perm or cfg.to_host(d_out, 32 * n) != twin_out:
                    raise SystemExit(f"fr_sort_bench.py: GPU and host twin differ: {dist} at 2^{log_n}")
                clk = shader_clock_mhz(cfg.device())
                clocks.append(clk)
                row = {"log_n": log_n, "distribution": dist, "digit_mask": "0x%08X" % mask, "plan": pkg.test_fr_sort_plan(n, 1, mask),
                       "device_kernel_ms": round(dev_kernel, 4), "device_call_ms": round(dev_wall, 4),
                       "host_kernel_ms": round(host_kernel, 4), "host_call_ms": round(host_wall, 4),
                       "host_twin_16_threads_ms": round(twin_ms, 2), "twin_over_device_call": round(twin_ms / dev_wall, 1),
                       "must_move_bytes": must_move(n, mask), "hbm_bound_ms": round(must_move(n, mask) / HBM_BYTES_PER_S * 1e3, 4),
                       "sclk_mhz": clk}
                rows.append(row)
                print(json.dumps(row), flush=True)
        # the permuted columns over a sorted handle at the largest size, on device buffers
        n = big
        rng = np.random.default_rng(7)
        table = np.zeros((n, 32), dtype=np.uint8)
        table[:, :3] = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)   # values below 2^24: duplicate rows
        idx = rng.integers(0, n, size=n)
        data = table[idx].tobytes()
        cfg.to_device(d_in, table.tobytes())
        t0 = time.perf_counter()
        h, _ = cfg.fr_lookup_build_sorted(d_in, layout, n, pkg.MEM_DEVICE, perm_out=d_perm)
        build_wall = (time.perf_counter() - t0) * 1e3
        d_a = cfg.alloc(32 * n)
        try:
            cfg.to_device(d_in, data)
            walls = {pkg.PERMUTE_ROWS: [], pkg.PERMUTE_HALO2: []}
            for k in range(2 * (args.warmup + args.iters)):           # alternated call by call
                how = (pkg.PERMUTE_ROWS, pkg.PERMUTE_HALO2)[k % 2]
                t0 = time.perf_counter()
                cfg.fr_lookup_permute_as(h, d_in, how, layout, 1, pkg.MEM_DEVICE, n=n, a_out=d_a, s_out=d_out)
                if k >= 2 * args.warmup:
                    walls[how].append(((time.perf_counter() - t0) * 1e3, cfg.last_kernel_ms))
            for how, name in ((pkg.PERMUTE_ROWS, "rows"), (pkg.PERMUTE_HALO2, "halo2")):
                permute_rows.append({"log_n": max(args.logs), "arrangement": name,
                                     "device_kernel_ms": round(statistics.median(w[1] for w in walls[how]), 4),
                                     "device_call_ms": round(statistics.median(w[0] for w in walls[how]), 4)})
                print(json.dumps(permute_rows[-1]), flush=True)
            permute_rows.append({"log_n": max(args.logs), "build_sorted_device_kernel_ms": round(h.build_ms, 4),
                                 "build_sorted_device_call_ms_first_call": round(build_wall, 4)})
            print(json.dumps(permute_rows[-1]), flush=True)
        finally:
            cfg.free(d_a)
            h.free()
        for p in (d_in, d_out, d_perm):
            cfg.free(p)
    finally:
        cfg.close()
    result = {
        "tool": "tools/fr_sort_bench.py", "device": "one MI355X", "commit": args.commit or commit(), "sclk_mhz": clocks,
        "iters": args.iters, "warmup": args.warmup, "prewarm_ms": args.prewarm_ms,
        "setting": "CANON_LE, one column, out and perm_out; kernel_ms as the call reports it, call time as wall time of the "
                   "blocking call, medians; no timing is a pass condition",
        "alternated": "permute_as HALO2 against ROWS, call by call; the sort itself has one form and was alternated against nothing",
        "rows": rows, "permute_as_device": permute_rows,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
