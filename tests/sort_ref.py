"""Model side of the sort tests (msm_amd_fr_sort, msm_amd_host_fr_sort): Python integers, and from np_records on a numpy
model for CANON_LE columns whose values are below 2^64 (tests/test_np_models_host.py pins it to the integer model).  A column is sorted with
Python's `sorted` on (value mod r, index), which is the stable ascending order by canonical value; a model call takes records
and returns records, so that a test compares bytes.  Also the digit mask of a call (which bytes of the little-endian residue
differ anywhere in it) and the plan that follows from a mask, from the definition in the header.  Nothing here calls the
library."""
import random

import numpy as np

from fr_ref import decode, encode, first_difference, raw, words  # noqa: F401
from ntt_ref import CANON_LE, LAYOUTS, MONT, MONT_LE, R  # noqa: F401

MEM_HOST, MEM_DEVICE = 0, 1                                   # MSM_AMD_MEM_*
TILE = 4096                                                   # pairs per tile of a pass; a wave owns a quarter
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 12305]
# fr_sort_row_scan_kernel scans a digit's counts over the tiles with 1024 threads: the second wave holds a count from 65 tiles on,
# the loop takes a second trip from 1025 tiles on (tests/test_gpu_many_workgroups.py; tests/test_thresholds_host.py recomputes both)
ROW_SCAN_THREADS, WAVE = 1024, 64
N_65_TILES = WAVE * TILE + 1                                  # 262 145: the 65th tile holds one pair
N_1025_TILES = ROW_SCAN_THREADS * TILE + 1                    # 4 194 305


def sort(data, layout, n_vec=1):
    """(sorted records, perm list) of n_vec columns back to back; perm is column-relative"""
    vals = decode(data, layout)
    n = len(vals) // n_vec if n_vec else 0
    out, perm = [], []
    for v in range(n_vec):
        col = vals[v * n:(v + 1) * n]
        order = [i for _, i in sorted((x, i) for i, x in enumerate(col))]
        perm += order
        out += [col[i] for i in order]
    return encode(out, layout), perm


def digit_mask(data, layout):
    """bit d: byte d of the little-endian residue differs from that of record 0 somewhere in the call"""
    vals = decode(data, layout)
    mask = 0
    for x in vals:
        diff = x ^ vals[0]
        for d in range(32):
            if (diff >> (8 * d)) & 0xFF:
                mask |= 1 << d
    return mask


def plan(n, n_vec, mask):
    """passes, launches, tiles of a sort (include/msm_amd.h, msm_amd_test_fr_sort_plan); bytes are not modelled"""
    passes = bin(mask).count("1")
    gathers = sum(1 for w in range(8) if (mask >> (4 * w)) & 0xF)
    return dict(passes=passes, launches=1 + n_vec * (gathers + 3 * passes + 1), tiles=-(-n // TILE))


def random_column(seed, n, layout, below=R):
    rng = random.Random(seed)
    return encode([rng.randrange(below) for _ in range(n)], layout)


def few_values(seed, n, layout, distinct):
    rng = random.Random(seed)
    pool = [rng.randrange(R) for _ in range(distinct)]
    return encode([rng.choice(pool) for _ in range(n)], layout)


def runs_ascend(data, perm, layout, n_vec=1):
    """perm ascends inside every run of equal values of the sorted columns, and the values ascend"""
    vals = decode(data, layout)
    n = len(vals) // n_vec
    for v in range(n_vec):
        col, p = vals[v * n:(v + 1) * n], perm[v * n:(v + 1) * n]
        assert sorted(p) == list(range(n))
        for k in range(1, n):
            a, b = col[p[k - 1]], col[p[k]]
            assert a < b or (a == b and p[k - 1] < p[k]), (v, k)


# ---- the numpy model: CANON_LE records of values below 2^64 as (n, 8) uint32 arrays ------------------------------------------------
def np_records(vals):
    """(n, 8) uint32 CANON_LE records of values below 2^64"""
    v = np.asarray(vals, dtype=np.uint64)
    rec = np.zeros((v.size, 8), dtype=np.uint32)
    rec[:, 0] = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rec[:, 1] = (v >> np.uint64(32)).astype(np.uint32)
    return rec


def np_values(rec):
    """the uint64 values of such records; a record with a word above the second is no input of this model"""
    rec = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 8)
    assert not rec[:, 2:].any()
    return rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))


def np_from_bytes(data):
    return np.frombuffer(data, dtype=np.uint32).reshape(-1, 8)


def np_sort(rec, n_vec=1):
    """sort() on such records: ((n_vec n, 8) sorted records, uint32 column-relative perm)"""
    keys = np_values(rec).reshape(n_vec, -1)
    perm = np.argsort(keys, axis=1, kind="stable")
    out = np.take_along_axis(keys, perm, axis=1)
    return np_records(out.reshape(-1)), perm.reshape(-1).astype(np.uint32)


def np_digit_mask(rec):
    """digit_mask() on such records"""
    b = np.ascontiguousarray(rec, dtype=np.uint32).reshape(-1, 8).view(np.uint8).reshape(-1, 32)
    differs = (b != b[0]).any(axis=0)
    return sum(1 << d for d in range(32) if differs[d])


def np_runs_ascend(rec, perm, n_vec=1):
    """runs_ascend() on such records and a uint32 perm array"""
    keys = np_values(rec).reshape(n_vec, -1)
    p = np.asarray(perm, dtype=np.int64).reshape(n_vec, -1)
    n = keys.shape[1]
    for v in range(n_vec):
        assert np.array_equal(np.sort(p[v]), np.arange(n))
        k = keys[v][p[v]]
        assert ((k[:-1] < k[1:]) | ((k[:-1] == k[1:]) & (p[v][:-1] < p[v][1:]))).all(), v
