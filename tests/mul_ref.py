"""Model side of the batch scalar multiplication tests (msm_amd_mul_points*, msm_amd_g2_mul_points*): expected points
from the big-integer models (oracle.bn254_ref for G1, g2_ref for G2; check_ref for the special G2 points and the record
encoders), the planted scalars, and the record encoders of every layout; the whole-array cases (scalar and base
progressions, every table entry, the digit edges) whose expected values are affine additions of the models, and the
G1 inputs that take the exceptional branches of the additions.  Nothing here calls the library."""
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
# s* = 96 2^248 - r: the one scalar below r (window 8, 32 windows) whose top signed digit d (48) and low 31 windows L
# satisfy L = d 2^248 (mod r), so that the last mixed addition of the digit walk meets acc == T[31][d - 1] and must double
# on ANY base of order r
S_STAR = 96 * (1 << 248) - R
assert 0 < S_STAR < R and S_STAR >> 248 == 0x2F and (S_STAR - (48 << 248)) % R == (48 << 248) % R


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
    if (cw, W) == (8, 32):
        cases.append((S_STAR, "s* = 96 2^248 - r"))
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


# ---- whole arrays from affine additions of the models ------------------------------------------------------------------------
def add(group, a, b):
    return o.aff_add(a, b) if group == 1 else g.add(a, b)


def neg(group, a):
    return o.aff_neg(a) if group == 1 else g.neg(a)


def progression(group, first, step, n):
    """first, first + step, ..., n points"""
    out = [first]
    for _ in range(n - 1):
        out.append(add(group, out[-1], step))
    return out


@functools.lru_cache(maxsize=None)
def random_base(group, seed=91):
    """a base that is not the generator (G2: inside the r-torsion)"""
    return random_points(group, 1, seed)[0]


@functools.lru_cache(maxsize=None)
def scalar_progression(group, n, seed=1234):
    """(scalars, base, expected points): s_i = (s_0 + i d) mod r on random_base; out[0] = [s_0] P by the model's scalar
    multiplication, out[i + 1] = out[i] + [d] P"""
    rng = random.Random(seed + group)
    s0, d = rng.getrandbits(254) % R, rng.getrandbits(254) % R
    base = random_base(group)
    ks = [(s0 + i * d) % R for i in range(n)]
    return ks, base, progression(group, expected(group, s0, base), expected(group, d, base), n)


@functools.lru_cache(maxsize=None)
def base_progression(group, s, n, seed=4321):
    """(bases, expected points): P_i = P_0 + i Q, out[i] = [s] P_0 + i [s] Q"""
    p0, q = random_points(group, 2, seed)[0], random_points(group, 2, seed + 1)[1]
    return progression(group, p0, q, n), progression(group, expected(group, s, p0), expected(group, s, q), n)


@functools.lru_cache(maxsize=None)
def multiples(group, pt, cw=8, W=32):
    """rows[w][d] = [d 2^(cw w)] pt for d = 0 .. 2^cw - 1 (rows[w][0] = None): additions inside a window, cw doublings
    between windows.  Entries 1 .. 2^(cw-1) of row w are the library's fixed-base table of pt."""
    rows, base = [], pt
    for _ in range(W):
        rows.append([None] + progression(group, base, base, (1 << cw) - 1))
        for _ in range(cw):
            base = add(group, base, base)
    return rows


def from_rows(group, rows, s, cw=8):
    """[s] pt from multiples(): one addition per non-zero window of the plain (unsigned) windows of s"""
    acc, w = None, 0
    while s:
        acc = add(group, acc, rows[w][s & ((1 << cw) - 1)])
        s >>= cw
        w += 1
    return acc


def whole_table_scalars(cw=8, W=32):
    """every d 2^(cw w) below r with d = 1 .. 2^cw - 1: d <= 2^(cw-1) reads table entry T[w][d - 1] and nothing else,
    a larger d reads T[w][2^cw - d - 1] negated and the carry entry T[w + 1][0].  (The top window holds d <= r >> 248 =
    48 only: no scalar layout delivers a larger value to the digit walk, it is reduced first.)"""
    ks = [d << (cw * w) for w in range(W) for d in range(1, 1 << cw) if d << (cw * w) < R]
    assert all(0 < k < R for k in ks) and len(set(ks)) == len(ks)
    assert len(ks) == (W - 1) * ((1 << cw) - 1) + (R >> (cw * (W - 1)))      # 31 x 255 + 48 = 7953
    return ks


def _lone_digit(k, cw):
    while k & ((1 << cw) - 1) == 0:
        k >>= cw
    assert k < 1 << cw
    return k


def digit_edge_scalars(cw=8, W=32, seed=5):
    """(scalars, names): the window values 2^(cw-1) - 1, 2^(cw-1), 2^(cw-1) + 1 and 2^cw - 1 (0x7F, 0x80, 0x81, 0xFF)
    alone in a window, with an incoming carry (the window below holds 0x81 or 0xFF), next to each other in two windows,
    and runs of 0xFF that carry through 4 and more windows into the top one"""
    assert (cw, W) == (8, 32)
    edges = (0x7F, 0x80, 0x81, 0xFF)
    rng = random.Random(seed)
    cases = []
    for w in (0, 1, 13, 30):
        for b in edges:
            cases.append((b << (8 * w), f"{b:#x} in window {w}"))
            if w:
                for low in (0x81, 0xFF):
                    cases.append(((b << (8 * w)) | (low << (8 * (w - 1))), f"{b:#x} in window {w}, carry from {low:#x}"))
    for w in (0, 17, 29):
        for b1 in edges:
            for b2 in edges:
                cases.append(((b1 << (8 * w)) | (b2 << (8 * (w + 1))) | (rng.randrange(1, 0x2F) << (8 * (w + 2))),
                              f"{b1:#x}, {b2:#x} in windows {w}, {w + 1}"))
    for run in (4, 5, 12, 31):                                   # windows 31 - run .. 30 hold 0xFF, the top one 0x2F -> 0x30
        ff = ((1 << (8 * run)) - 1) << (8 * (31 - run))
        low = rng.getrandbits(8 * (31 - run)) if run < 31 else 0
        cases.append(((0x2F << 248) | ff | low, f"{run} windows of 0xff carry into the top one"))
        cases.append(((0x01 << 248) | ff | low, f"{run} windows of 0xff carry into the top one (1 -> 2)"))
    cases.append(((0x2F << 248) | (((1 << 32) - 1) << 216) | (0x81 << 208), "0x81 below 4 windows of 0xff below the top"))
    assert all(0 < k < R for k, _ in cases)
    return [k for k, _ in cases], [nm for _, nm in cases]


@functools.lru_cache(maxsize=None)
def table_case(group, cw=8, W=32):
    """(scalars, names, base, expected points) of the whole-table and digit-edge scalars on random_base, every expected
    value from multiples()"""
    base = random_base(group)
    rows = multiples(group, base, cw, W)
    ks = whole_table_scalars(cw, W)
    names = [f"{_lone_digit(k, cw)} 2^{(k.bit_length() - 1) // cw * cw}" for k in ks]
    eks, enames = digit_edge_scalars(cw, W)
    ks, names = ks + eks, names + enames
    return ks, names, base, [from_rows(group, rows, k, cw) for k in ks]


def star_scalars():
    """(stored integers, reduced scalars): s*, s* - 1, s* + 1, and s* as s* + r and s* + 4 r (canonical layouts only)"""
    stored = [S_STAR, S_STAR - 1, S_STAR + 1, S_STAR + R, S_STAR + 4 * R]
    assert max(stored) < 1 << 256
    return stored, [k % R for k in stored]


def star_bases(group):
    """(base, scalar layouts to run it under): the generator under all three, two random bases under one canonical
    layout each (only those can store s* + r)"""
    pts = random_points(group, 2, 77)
    return [(GEN[group], (1, 2, 0)), (pts[0], (1,)), (pts[1], (2,))]


ORDER3_Y = (5, 0x1F3D5A7C9B2E4F60718293A4B5C6D7E8F9012345)      # (0, y) on y^2 = x^3 + y^2: any y != 0 serves


def order3_scalars(seed=33):
    rng = random.Random(seed)
    return list(range(10)) + [R - 1, S_STAR] + [rng.randrange(R) for _ in range(32)]
