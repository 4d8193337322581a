"""Model side of the permuted-columns tests (msm_amd_fr_lookup_permute*): Python integers only.  permute() is the definition
of include/msm_amd.h written out -- counters credited to the representative row, groups in row order, the unused rows in
ascending order -- and check_halo2() tests what halo2's verifier asks of A' and S' directly, without the model.  A model
call takes records and returns records, so that a test compares bytes.  Nothing here calls the library."""
import random
from collections import Counter

import lookup_ref as lr
from fr_ref import decode, encode, first_difference, raw  # noqa: F401
from lookup_ref import CANON_LE, LAYOUTS, MONT_LE, NO_MISS, R  # noqa: F401

DEFAULT_TILE_LOG = 11                                              # kPermuteTileLog
# n_rows round the shipped tile and well into its second level (tests/test_gpu_many_workgroups.py); the third level starts
# above 2^22 rows and is reached with MSM_AMD_PERMUTE_TILE_LOG only
SHIPPED_TILE_SIZES = (2047, 2048, 2049, (1 << 16) + 3)


def permute(table, data, layout, n_vec=1, want_s=True):
    """(A' records or None, S' records or None, report dict): both None if a value is in no row (the call fails and leaves
    its outputs).  S' only for n == n_rows."""
    rep = lr.representatives(table, layout)
    rows = decode(table, layout)
    n_rows, vals = len(rows), decode(data, layout)
    total = len(vals)
    n = total // n_vec if n_vec else 0
    missing = [i for i, v in enumerate(vals) if v not in rep]
    a_all, s_all, rows_hit, most = [], [], 0, 0
    for v in range(n_vec):
        c = [0] * n_rows
        for x in vals[v * n:(v + 1) * n]:
            if x in rep:
                c[rep[x]] += 1
        rows_hit += sum(1 for k in c if k)
        most = max(most, max(c))
        if missing:
            continue
        unused = iter([j for j in range(n_rows) if c[j] == 0])
        for j in range(n_rows):
            a_all += [rows[j]] * c[j]
            if want_s and c[j]:
                s_all += [rows[j]] + [rows[next(unused)] for _ in range(c[j] - 1)]
    report = dict(n_missing=len(missing), first_missing=missing[0] if missing else (NO_MISS if total else 0),
                  rows_hit=rows_hit, max_multiplicity=most)
    if missing or not total:
        return None, None, report
    assert not want_s or n == n_rows
    return encode(a_all, layout), (encode(s_all, layout) if want_s else None), report


def check_halo2(a, table, a_perm, s_perm, layout, n_vec=1):
    """the constraints of halo2's lookup argument on every column: A' a permutation of A and S' of S as multisets of
    residues, A'[0] = S'[0], A'[i] = S'[i] or A'[i] = A'[i-1]; every output record fully reduced"""
    A, S, Ap, Sp = (decode(x, layout) for x in (a, table, a_perm, s_perm))
    assert a_perm == encode(Ap, layout) and s_perm == encode(Sp, layout), "an output record is not fully reduced"
    n = len(S)
    assert len(A) == len(Ap) == len(Sp) == n * n_vec
    for v in range(n_vec):
        lo = v * n
        assert Counter(Ap[lo:lo + n]) == Counter(A[lo:lo + n]), "A' is no permutation of A (column %d)" % v
        assert Counter(Sp[lo:lo + n]) == Counter(S), "S' is no permutation of S (column %d)" % v
        assert Ap[lo] == Sp[lo], "A'[0] != S'[0] (column %d)" % v
        for i in range(lo + 1, lo + n):
            assert Ap[i] == Sp[i] or Ap[i] == Ap[i - 1], "row %d of column %d" % (i - lo, v)


def product_closes(a, table, a_perm, s_perm, layout, beta, gamma):
    """prod (A + beta)(S + gamma) / ((A' + beta)(S' + gamma)) over one column, with big integers: 1 iff the column z closes"""
    num = den = 1
    for x, s, xp, sp in zip(*(decode(v, layout) for v in (a, table, a_perm, s_perm))):
        num = num * (x + beta) * (s + gamma) % R
        den = den * (xp + beta) * (sp + gamma) % R
    return num * pow(den, -1, R) % R == 1


def plan(n_rows, n_vec, tile_log):
    """msm_amd_test_fr_permute_plan restated: levels of the scan, kernels of a call, first-level tiles, bytes of workspace"""
    lens, length = [], n_rows
    while True:
        tiles = -(-length // (1 << tile_log))
        lens.append((length, tiles))
        if tiles <= 1:
            break
        length = tiles
    levels, cells = len(lens), n_rows * n_vec
    totals = sum(length for length, _ in lens[1:]) * n_vec
    nbytes = -(-cells * 4 // 16) * 16 + 64 + 8 * cells + 8 * totals + 4 * cells
    return dict(levels=levels, launches=2 * levels - 1 + 2, tiles=lens[0][1] * n_vec, bytes=nbytes)


# ---- input columns --------------------------------------------------------------------------------------------------------------
def column(kind, seed, table, layout, n):
    """n records over the rows of a table: 'uniform' draws, 'row<j>' that row n times, 'half' every other record row 0 and
    uniform draws between, 'shuffle' the table's rows in random order (n == n_rows)"""
    rng = random.Random(seed)
    rows = decode(table, layout)
    if kind == "uniform":
        vals = [rng.choice(rows) for _ in range(n)]
    elif kind.startswith("row"):
        vals = [rows[int(kind[3:]) % len(rows)]] * n
    elif kind == "half":
        vals = [rows[0] if i % 2 else rng.choice(rows) for i in range(n)]
    else:
        assert kind == "shuffle" and n == len(rows)
        vals = rows[:]
        rng.shuffle(vals)
    return encode(vals, layout)
