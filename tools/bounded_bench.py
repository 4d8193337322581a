#!/usr/bin/env python3
"""Time the bounded-width MSM (msm_amd_msm_bounded_device, msm_amd_msm_batch_bounded_device) and the width scan on one
GPU.

Device-resident prepared bases, uniformly random scalars below 2^bits (MSM_AMD_SCALAR_CANON_LE); every cell is timed lone
(one blocking call with nothing in flight) and pipelined (a blocking batch of --batch instances, time per MSM) and set
against the UNBOUNDED call on the same scalars and bases in the same run, the two alternated call by call.  A row holds
the medians, min and max of --iters calls after --warmup more, the windows both calls chose, the ratio of the times and
the counted ideal: the ratio of the window counts.  Signed rows: +-values below 2^bits, the negative ones as r - k.
The width scan is timed as the wall time of its blocking call against MSM_AMD_FR_MUL on the same count (same bytes in,
one product per record).
--sweep: instead, every forced window 3..17 per cell, as text (profiles/bounded_sweep.txt): what the window policy of
auto_window_bounded (msm_plan.hip) was read from.

  python tools/bounded_bench.py [--logs 16 20 22] [--bits 1 8 16 32 64 128 254] [--out profiles/bounded_bench.json]
  python tools/bounded_bench.py --sweep [--logs 16 18 20 22] [--out profiles/bounded_sweep.txt]
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
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
CANON = 1


def scalars_below(n, bits, seed, signed=False):
    """n CANON_LE records below 2^bits; signed: half of them as r - k"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    full, part = divmod(bits, 8)
    raw[:, full + (1 if part else 0):] = 0
    if part:
        raw[:, full] &= (1 << part) - 1
    if bits >= 254:
        raw[:, 31] &= 0x1F   # below 2^253 < r
    if signed:
        r_le = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint8).astype(np.int64)
        neg = rng.integers(0, 2, size=n).astype(bool)
        diff = r_le[None, :] - raw.astype(np.int64)
        for j in range(31):   # borrow ripple, byte by byte
            under = diff[:, j] < 0
            diff[under, j] += 256
            diff[under, j + 1] -= 1
        raw[neg] = diff[neg].astype(np.uint8)
    return raw.tobytes()


def stats(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples)}


def alternate(calls, warmup, iters):
    """the calls in turn, call by call: {name: [ms]}"""
    out = {k: [] for k in calls}
    for it in range(warmup + iters):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            if it >= warmup:
                out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def prewarm(cfg, ds, dp, n, seconds=1.0):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        cfg.msm_batch_device([ds] * 4, [dp] * 4, [n] * 4, scalar_layout=CANON, point_layout=4)


class Instance:
    def __init__(self, pkg, cfg, log_n):
        self.cfg, self.n = cfg, 1 << log_n
        dp, ds = cfg.generate_instance(0xB2540000 + log_n, self.n, True)
        self.bases = cfg.bases_prepare_device(dp, self.n)
        cfg.free(dp)
        cfg.free(ds)
        self.scalars = {}

    def device_scalars(self, bits, signed=False):
        key = (bits, signed)
        if key not in self.scalars:
            data = scalars_below(self.n, bits, 1000 + bits + (7 if signed else 0), signed)
            d = self.cfg.alloc(len(data))
            self.cfg.to_device(d, data)
            self.scalars[key] = d
        return self.scalars[key]

    def close(self):
        for d in self.scalars.values():
            self.cfg.free(d)
        self.cfg.free(self.bases)


def cell(pkg, cfg, inst, bits, sign, batch, warmup, iters):
    """lone and pipelined, bounded against unbounded, at whatever window the ctx picks or was forced to"""
    n, dp = inst.n, inst.bases
    ds = inst.device_scalars(bits, bool(sign))
    row = {}
    lone = alternate({
        "bounded": lambda: cfg.msm_bounded_device(ds, dp, n, bits, sign, scalar_layout=CANON, point_layout=pkg.POINT_PREPARED),
        "unbounded": lambda: cfg.msm_batch_device([ds], [dp], [n], scalar_layout=CANON, point_layout=pkg.POINT_PREPARED),
    }, warmup, iters)
    piped = alternate({
        "bounded": lambda: cfg.msm_batch_bounded_device([ds] * batch, [dp] * batch, [n] * batch, bits, sign, scalar_layout=CANON,
                                                        point_layout=pkg.POINT_PREPARED),
        "unbounded": lambda: cfg.msm_batch_device([ds] * batch, [dp] * batch, [n] * batch, scalar_layout=CANON,
                                                  point_layout=pkg.POINT_PREPARED),
    }, warmup, iters)
    for mode, res, per in (("lone", lone, 1), ("pipelined", piped, batch)):
        row[mode] = {k: stats([v / per for v in vs]) for k, vs in res.items()}
    return row


def windows_of(pkg, n, bits, lone, forced=0):
    cb = forced or pkg.auto_window_size_bounded(n, bits, lone)
    cu = forced or pkg.auto_window_size_bounded(n, 254, lone)
    return cb, bits // cb + 1, cu, 254 // cu + 1


def run_bench(pkg, cfg, args):
    rows, scans = [], []
    for log_n in args.logs:
        inst = Instance(pkg, cfg, log_n)
        prewarm(cfg, inst.device_scalars(254), inst.bases, inst.n)
        batch = max(2, min(args.batch, (1 << 24) >> log_n))
        for sign in (0, 1):
            for bits in args.bits:
                if sign and bits > 253 or sign and bits not in (8, 32, 64):
                    continue
                res = cell(pkg, cfg, inst, bits, sign, batch, args.warmup, args.iters)
                for mode in ("lone", "pipelined"):
                    cb, wb, cu, wu = windows_of(pkg, inst.n, bits, mode == "lone")
                    b, u = res[mode]["bounded"], res[mode]["unbounded"]
                    spread = max(b["max_ms"] - b["min_ms"], u["max_ms"] - u["min_ms"])
                    rows.append({"log_n": log_n, "bits": bits, "signed": bool(sign), "mode": mode, "batch": batch if mode == "pipelined" else 1,
                                 "bounded": b, "unbounded": u, "ratio": b["median_ms"] / u["median_ms"],
                                 "window_bounded": cb, "windows_bounded": wb, "window_unbounded": cu, "windows_unbounded": wu,
                                 "ideal_ratio": wb / wu, "faster_by_more_than_spread": u["median_ms"] - b["median_ms"] > spread})
                    print(json.dumps(rows[-1]), flush=True)
        inst.close()
    for log_n in args.scan_logs:
        n = 1 << log_n
        data = scalars_below(n, 64, 5)
        d, out = cfg.alloc(len(data)), cfg.alloc(len(data))
        cfg.to_device(d, data)
        kernel = []
        res = alternate({
            "scalar_width": lambda: cfg.scalar_width_device(d, n, 1, CANON),
            "fr_mul": lambda: kernel.append(cfg.fr_map_device(pkg.FR_MUL, d, d, None, n, out, scalar_layout=CANON)),
        }, args.warmup, args.iters)
        row = {"log_n": log_n, "scalar_width_wall": stats(res["scalar_width"]), "fr_mul_wall": stats(res["fr_mul"]),
               "fr_mul_kernel_ms": statistics.median(kernel[-args.iters:])}
        row["wall_ratio"] = row["scalar_width_wall"]["median_ms"] / row["fr_mul_wall"]["median_ms"]
        scans.append(row)
        print(json.dumps(row), flush=True)
        cfg.free(d)
        cfg.free(out)
    return {"host": socket.gethostname(), "version": pkg.lib().msm_amd_version().decode(), "iters": args.iters,
            "warmup": args.warmup, "msm": rows, "width_scan": scans}


def run_sweep(pkg, cfg, args):
    lines = ["# bounded-width window sweep: median ms per MSM (min-max) of %d calls; lone = one blocking call, pipelined = a"
             % args.iters, "# blocking batch; prepared bases, random CANON_LE scalars below 2^bits; '*' = fastest of the row's mode",
             "# host %s, %s" % (socket.gethostname(), pkg.lib().msm_amd_version().decode())]
    for log_n in args.logs:
        inst = Instance(pkg, cfg, log_n)
        prewarm(cfg, inst.device_scalars(254), inst.bases, inst.n)
        batch = max(2, min(args.batch, (1 << 24) >> log_n))
        n, dp = inst.n, inst.bases
        for bits in args.bits:
            ds = inst.device_scalars(bits)
            found = {"lone": {}, "pipelined": {}}
            for c in range(3, 18):
                if (bits // c + 1) * n > 1 << 27:   # a window two orders of magnitude off: not measured
                    continue
                cfg.set_window_size(c)
                calls = {"lone": (lambda: cfg.msm_bounded_device(ds, dp, n, bits, 0, scalar_layout=CANON, point_layout=pkg.POINT_PREPARED), 1),
                         "pipelined": (lambda: cfg.msm_batch_bounded_device([ds] * batch, [dp] * batch, [n] * batch, bits, 0,
                                                                            scalar_layout=CANON, point_layout=pkg.POINT_PREPARED), batch)}
                for mode, (call, per) in calls.items():
                    t0 = time.perf_counter()
                    call()
                    first = (time.perf_counter() - t0) * 1e3 / per
                    if first > args.skip_above_ms:   # a window that is an order of magnitude off: one call is enough
                        found[mode][c] = {"median_ms": first, "min_ms": first, "max_ms": first}
                        continue
                    found[mode][c] = stats([v / per for v in alternate({"x": call}, 1, args.iters)["x"]])
            cfg.set_window_size(0)
            for mode in ("lone", "pipelined"):
                best = min(found[mode], key=lambda c: found[mode][c]["median_ms"])
                policy = pkg.auto_window_size_bounded(n, bits, mode == "lone")
                cells = " ".join("c=%d%s %.3f(%.3f-%.3f)" % (c, "*" if c == best else "", r["median_ms"], r["min_ms"], r["max_ms"])
                                 for c, r in sorted(found[mode].items()))
                lines.append("2^%d bits=%d %s policy=c%d: %s" % (log_n, bits, mode, policy, cells))
                print(lines[-1], flush=True)
        inst.close()
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+")
    ap.add_argument("--bits", type=int, nargs="+")
    ap.add_argument("--scan-logs", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-above-ms", type=float, default=40.0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    try:
        if args.sweep:
            args.logs = args.logs or [16, 18, 20, 22]
            args.bits = args.bits or [1, 8, 16, 32, 64, 128]
            text = run_sweep(pkg, cfg, args)
            with open(args.out or os.path.join(ROOT, "profiles", "bounded_sweep.txt"), "w") as f:
                f.write(text)
        else:
            args.logs = args.logs or [16, 20, 22]
            args.bits = args.bits or [1, 8, 16, 32, 64, 128, 254]
            result = run_bench(pkg, cfg, args)
            with open(args.out or os.path.join(ROOT, "profiles", "bounded_bench.json"), "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    finally:
        cfg.close()


if __name__ == "__main__":
    main()
