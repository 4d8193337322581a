"""Model side of the value-order arrangement of the permuted lookup columns (MSM_AMD_PERMUTE_HALO2 of
msm_amd_fr_lookup_permute_as): upstream's permute_expression_pair (halo2_proofs, plonk/lookup/prover.rs) written out step by
step with Python integers -- the sorted input column, the leftover table multiset kept in value order, the rows of repeated
inputs remembered and handed out from the LAST one down.  It is the literal algorithm, not the reduction to the row-order
pipeline over a sorted table that the library uses.  The report is that of tests/permute_ref.py (it does not depend on the
arrangement).  Nothing here calls the library."""
import json
import os

import lookup_ref as lr
import permute_ref as pr
from fr_ref import decode, encode, first_difference, raw  # noqa: F401
from lookup_ref import CANON_LE, LAYOUTS, MONT_LE, NO_MISS, R  # noqa: F401

ROWS, HALO2 = 0, 1                                            # MSM_AMD_PERMUTE_*
KNOWN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permute_halo2_known.json")


def permute_values(A, S):
    """(A', S') of one column of integers, or None if a value of A is not in S"""
    permuted_input = sorted(A)
    leftover = {}
    for s in S:
        leftover[s] = leftover.get(s, 0) + 1
    permuted_table = [None] * len(A)
    repeated_input_rows = []
    for row, value in enumerate(permuted_input):
        if row == 0 or value != permuted_input[row - 1]:
            permuted_table[row] = value
            if leftover.get(value, 0) == 0:
                return None
            leftover[value] -= 1
        else:
            repeated_input_rows.append(row)
    for element in sorted(leftover):
        for _ in range(leftover[element]):
            permuted_table[repeated_input_rows.pop()] = element
    assert not repeated_input_rows
    return permuted_input, permuted_table


def permute(table, data, layout, n_vec=1, want_s=True):
    """(A' records or None, S' records or None, report dict), as permute_ref.permute; S' needs n == n_rows"""
    report = pr.permute(table, data, layout, n_vec, want_s=False)[2]
    vals, S = decode(data, layout), decode(table, layout)
    n = len(vals) // n_vec if n_vec else 0
    if report["n_missing"] or not vals:
        return None, None, report
    a_all, s_all = [], []
    for v in range(n_vec):
        col = vals[v * n:(v + 1) * n]
        if want_s:
            assert n == len(S)
            a, s = permute_values(col, S)
            s_all += s
        else:
            a = sorted(col)
        a_all += a
    return encode(a_all, layout), (encode(s_all, layout) if want_s else None), report


def known():
    with open(KNOWN) as f:
        return json.load(f)
