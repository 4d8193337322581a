"""Model side of the sort tests (msm_amd_fr_sort, msm_amd_host_fr_sort): Python integers only.  A column is sorted with
Python's `sorted` on (value mod r, index), which is the stable ascending order by canonical value; a model call takes records
and returns records, so that a test compares bytes.  Also the digit mask of a call (which bytes of the little-endian residue
differ anywhere in it) and the plan that follows from a mask, from the definition in the header.  Nothing here calls the
library."""
import random

from fr_ref import decode, encode, first_difference, raw, words  # noqa: F401
from ntt_ref import CANON_LE, LAYOUTS, MONT, MONT_LE, R  # noqa: F401

MEM_HOST, MEM_DEVICE = 0, 1                                   # MSM_AMD_MEM_*
TILE = 4096                                                   # pairs per tile of a pass; a wave owns a quarter
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 12305]


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
