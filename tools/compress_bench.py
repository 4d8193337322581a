#!/usr/bin/env python3
"""Compressed-point timing on one ctx: one JSON line with, per size (2^16, 2^18, 2^20), group (G1, G2) and format (ARK,
PARITY), the median / min / max ms of blocking device-resident calls -- decompress straight to *_PREPARED records, and
compress from halo2curves affine records -- with the kernel time of the median call, the host twins at 16 threads on the
same inputs (one run each, to affine records: the twins have no prepared form), and the upload of the affine array the
decompression replaces (copy_to_device of n x 64 B / n x 128 B from pageable memory, median).
Usage: python tools/compress_bench.py [--reps R] [--sizes 16,18,20] [--no-host] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--no-host", action="store_true", help="skip the host twins")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import g2_ref as g
    from oracle import bn254_ref as o
    pkg = importlib.import_module("metal-msm-gpu-acceleration_amd")
    cfg = pkg.setup_metal_state(0)
    res = {"metric": "compress_points_ms", "reps": args.reps, "host_threads": 16, "sizes": {}}

    def stats(ms, kernel=None):
        out = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
        if kernel is not None:
            out["kernel_ms"] = round(kernel[sorted(range(len(ms)), key=lambda i: ms[i])[len(ms) // 2]], 3)
        return out

    def series(fn, kernel_of=None):
        fn()                                     # warm-up (allocations)
        ms, dev = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rep = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            if kernel_of:
                dev.append(kernel_of(rep))
        return stats(ms, dev if kernel_of else None)

    def once(fn):
        t0 = time.perf_counter()
        fn()
        return round((time.perf_counter() - t0) * 1e3, 1)

    def valid(rep):
        assert rep["n_invalid"] == 0, rep
        return rep["device_ms"]

    try:
        for logn in (int(s) for s in args.sizes.split(",")):
            n = 1 << logn
            affine = {1: pkg.generate_instance_host(o.SEED_BASE, n)[0],
                      2: pkg.g2_progression(g.encode_h2c(g.scalar_mul(3, g.GEN2)), g.encode_h2c(g.scalar_mul(5, g.GEN2)), n)}
            entry = {}
            for group in (1, 2):
                g2 = group == 2
                prepared = pkg.G2_POINT_PREPARED if g2 else pkg.POINT_PREPARED
                d_aff = cfg.alloc(len(affine[group]))
                d_prep = cfg.alloc(n * pkg.decompressed_bytes(prepared, g2))
                d_comp = cfg.alloc(n * (64 if g2 else 32))
                e = {"upload_affine_ms": series(lambda: cfg.to_device(d_aff, affine[group]))}
                for fmt, name in ((pkg.COMPRESSED_ARK, "ark"), (pkg.COMPRESSED_PARITY, "parity")):
                    e[f"{name}_compress_ms"] = series(lambda: cfg.compress_points_device(d_aff, n, d_comp, fmt, 0, g2=g2))
                    e[f"{name}_decompress_to_prepared_ms"] = series(
                        lambda: cfg.decompress_points_device(d_comp, n, d_prep, fmt, prepared, g2=g2), valid)
                    if not args.no_host:
                        comp = cfg.to_host(d_comp, n * (64 if g2 else 32))
                        e[f"host_{name}_decompress_ms"] = once(
                            lambda: pkg.host_decompress_points(comp, n, fmt, 0, g2=g2, threads=16, reasons=False))
                        e[f"host_{name}_compress_ms"] = once(
                            lambda: pkg.host_compress_points(affine[group], n, fmt, 0, g2=g2, threads=16))
                for p in (d_aff, d_prep, d_comp):
                    cfg.free(p)
                entry["g2" if g2 else "g1"] = e
            res["sizes"][f"2^{logn}"] = entry
    finally:
        cfg.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
