"""Model side of the lookup tests (msm_amd_fr_lookup_*, msm_amd_fr_prefix_sum*, msm_amd_fr_shift*): Python integers only.
A table is a dict from residue to the smallest row index that holds it; the multiplicities are credited to that row; the
row indices, the report, the running sums and the shift.  A model call takes records and returns records, so that a test
compares bytes.  Nothing here calls the library."""
import random

from fr_ref import EXCLUSIVE, INCLUSIVE, decode, encode, first_difference, raw, words  # noqa: F401
from ntt_ref import CANON_LE, LAYOUTS, MONT, MONT_LE, R  # noqa: F401

STRICT, COUNT_MISSING = 0, 1                                 # MSM_AMD_LOOKUP_*
NOT_FOUND = 0xFFFFFFFF
NO_MISS = (1 << 64) - 1
EDGE_WORDS = (0, 1, R - 1, R, R + 5, (1 << 256) - 1)          # 256-bit words as they stand in a record


def edge_records(layout):
    """records whose WORDS are the edge words: in MONT_LE the word w stands for w / MONT, in CANON_LE for w, both mod r"""
    return raw(EDGE_WORDS)


def representatives(table, layout):
    rep = {}
    for j, v in enumerate(decode(table, layout)):
        rep.setdefault(v, j)
    return rep


def multiplicities(table, data, layout, on_missing=COUNT_MISSING):
    """(m records or None, idx list, report dict): m is None for a miss under STRICT (the call fails and leaves m_out)"""
    rep = representatives(table, layout)
    n_rows = len(table) // 32
    counts = [0] * n_rows
    idx, missing, first = [], 0, NO_MISS
    for i, v in enumerate(decode(data, layout)):
        j = rep.get(v, NOT_FOUND)
        idx.append(j)
        if j == NOT_FOUND:
            missing += 1
            first = min(first, i)
        else:
            counts[j] += 1
    total = len(idx)
    report = dict(n_missing=missing, first_missing=first if total else 0, rows_hit=sum(1 for c in counts if c),
                  max_multiplicity=max(counts))
    m = None if (on_missing == STRICT and missing) else encode(counts, layout)
    return m, idx, report


def n_distinct(table, layout):
    return len(representatives(table, layout))


def prefix_sum(data, layout, mode, n_vec=1):
    vals = decode(data, layout)
    n = len(vals) // n_vec if n_vec else 0
    out = []
    for v in range(n_vec):
        run = 0
        for x in vals[v * n:(v + 1) * n]:
            if mode == EXCLUSIVE:
                out.append(run)
            run = (run + x) % R
            if mode == INCLUSIVE:
                out.append(run)
    return encode(out, layout)


def shift(a, k, layout):
    K = decode(k, layout)[0]
    return encode([x + K for x in decode(a, layout)], layout)


def random_table(seed, n_rows, layout, distinct=None):
    """n_rows records over `distinct` random values (default: all different), in random order"""
    rng = random.Random(seed)
    pool = [rng.randrange(R) for _ in range(distinct or n_rows)]
    vals = pool + [rng.choice(pool) for _ in range(n_rows - len(pool))]
    rng.shuffle(vals)
    return encode(vals, layout)


def draws(seed, table, layout, n, miss_at=()):
    """n records drawn from the rows of a table; the positions in miss_at hold values that are in no row"""
    rng = random.Random(seed)
    rows = decode(table, layout)
    have = set(rows)
    vals = [rng.choice(rows) for _ in range(n)]
    for i in miss_at:
        v = rng.randrange(R)
        while v in have:
            v = rng.randrange(R)
        vals[i] = v
    return encode(vals, layout)
