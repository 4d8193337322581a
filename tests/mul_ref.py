"""Model side of the batch scalar multiplication tests (msm_amd_mul_points*, msm_amd_g2_mul_points*): expected points
from the big-integer models (oracle.bn254_ref for G1, g2_ref for G2; check_ref for the special G2 points and the record
encoders), the planted scalars, and the record encoders of every layout.  Nothing here calls the library."""
import functools
import random

import check_ref as c
import g2_ref as g
from oracle import bn254_ref as o

R = o.R_ORDER
EACH, ONE = 0, 1                                            # MSM_AMD_MUL_BASE_*
SCALAR_LAYOUTS = (0, 1, 2)                                  # MONT_LE, CANON_LE, CANON_BE32
IN_LAYOUTS = {1: (c.H2C, c.ARK_PROJECTIVE, c.ARK_AFFINE, c.JAC_BE32), 2: (c.G2_H2C, c.G2_ARK)}
OUT_LAYOUTS = {1: (c.H2C, c.ARK_AFFINE), 2: (c.G2_H2C, c.G2_ARK)}
IN_BYTES = {1: c.G1_BYTES, 2: c.G2_BYTES}
OUT_BYTES = {(1, c.H2C): 64, (1, c.ARK_AFFINE): 72, (2, c.G2_H2C): 128, (2, c.G2_ARK): 136}
GEN = {1: o.GEN, 2: g.GEN2}
ORDER_SMALL = 10069


@functools.lru_cache(maxsize=None)
def expected(group, s, pt):
    """[s mod r] pt as an affine point, None = identity (s is what a canonical layout stores: the library reduces it)"""
    s %= R
    if pt is None or s == 0:
        return None
    if group == 1:
        return o.scalar_mul(s, pt)               # G1 has prime order r: the model's own reduction changes nothing
    return g.scalar_mul(s, pt)                   # integer multiple: right for points outside the r-torsion too


def base_record(group, layout, pt, z=1):
    """one base record of an input layout (None = the layout's identity encoding); G1 Jacobian layouts: with that Z"""
    return (c.g1_rec(layout, pt, z) if group == 1 else c.g2_rec(layout, pt)).encode()


def out_record(group, layout, pt):
    """one output record (an affine host layout): canonical coordinates, None = the layout's identity encoding"""
    return (c.g1_rec(layout, pt) if group == 1 else c.g2_rec(layout, pt)).encode()


def scalars_bytes(ks, layout):
    """canonical layouts store the integer as given (it may exceed r), the Montgomery layout stores k mod r"""
    return b"".join(g.encode_scalar(k, layout) for k in ks)


def planted_scalars(cw, W):
    """(scalars, names): the planted scalars for a fixed-base table of window cw bits and W windows"""
    cases = [(0, "0"), (1, "1"), (2, "2"), (R - 1, "r - 1"), ((R - 1) // 2, "(r - 1) / 2"), ((R + 1) // 2, "(r + 1) / 2")]
    for w in range(1, W):
        k = cw * w
        cases += [(1 << k, f"2^{k}"), ((1 << k) - 1, f"2^{k} - 1")]
    top = cw * (W - 1)
    # window W - 2 holds 2^(cw-1) + 1 > half: its digit goes negative and carries into the top window
    cases.append(((5 << top) | (((1 << (cw - 1)) + 1) << (top - cw)) | 123, "carry into the top window"))
    cases.append(((1 << 253) - 1, "2^253 - 1"))
    assert all(0 <= s < R for s, _ in cases)
    return [s for s, _ in cases], [nm for _, nm in cases]


def small_order_point():
    return c.special_g2()["order_10069"]


def random_points(group, n, seed):
    return c.g1_points(n, seed) if group == 1 else c.g2_points(n, seed)


def normalisation_case(K, n, seed, whole_group=False):
    """n small scalars (cheap for the model) with zeros -- identity results -- at positions 0, K - 1, K and n - 1 where
    they exist; whole_group: every scalar of the second group (or of the only one) is zero as well"""
    rng = random.Random(seed)
    ks = [rng.randrange(1, 1 << 48) for _ in range(n)]
    for i in (0, K - 1, K, n - 1):
        if 0 <= i < n:
            ks[i] = 0
    if whole_group:
        first = K if n > K else 0
        for i in range(first, min(n, first + K)):
            ks[i] = 0
    return ks
