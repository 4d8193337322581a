"""Model side of the multi-point tests (msm_amd_fr_poly_eval_points, msm_amd_fr_poly_div_points): Python integers on the
record coders of tests/fr_ref.py.  The division is schoolbook long division by the expanded vanishing polynomial
Z_S(X) = prod_j (X - z_j), the evaluation is Horner: neither the partial fractions of the device nor the chained linear
divisions of the host twin.  A model call takes records and returns records, so that a test compares bytes.  Nothing here
calls the library."""
import random

import poly_ref as p
from fr_ref import CANON_LE, LAYOUTS, MONT_LE, R, decode, encode, first_difference, random_values, raw, words  # noqa: F401

MAX_POINTS = 8                                   # MSM_AMD_POLY_MAX_POINTS
MEM_HOST, MEM_DEVICE = 0, 1                      # MSM_AMD_MEM_*
OMEGA_20 = pow(5, (R - 1) >> 20, R)              # of order 2^20: 5 generates Fr*, and 2^28 divides r - 1


def point_values(z_recs, layout):
    return decode(z_recs, layout)


def vanishing(zs):
    """the coefficients of prod_j (X - z_j), lowest degree first: monic of degree len(zs)"""
    poly = [1]
    for z in zs:
        nxt = [0] * (len(poly) + 1)
        for i, c in enumerate(poly):
            nxt[i + 1] = (nxt[i + 1] + c) % R
            nxt[i] = (nxt[i] - c * z) % R
        poly = nxt
    return poly


def long_division(coeffs, divisor):
    """schoolbook: (the floor quotient padded with zeros to len(coeffs), the remainder of len(divisor) - 1 coefficients);
    the divisor is monic"""
    n, k = len(coeffs), len(divisor) - 1
    rem, q = list(coeffs), [0] * n
    for i in range(n - 1, k - 1, -1):
        lead = rem[i]
        q[i - k] = lead
        if lead:
            for t in range(k + 1):
                rem[i - k + t] = (rem[i - k + t] - lead * divisor[t]) % R
    return q, (rem[:k] + [0] * k)[:k]


def div_points_ints(coeffs, zs):
    """(quotient of n coefficients, [p(z_j)])"""
    q, _ = long_division(coeffs, vanishing(zs))
    return q, [p.eval_ints(coeffs, z) for z in zs]


def eval_points(data, z_recs, layout, n_vec=1):
    """records of y[v k + j] = p_v(z_j)"""
    zs = point_values(z_recs, layout)
    return encode([p.eval_ints(c, z) for c in p.vectors(data, layout, n_vec) for z in zs], layout)


def div_points(data, z_recs, layout, n_vec=1):
    """(records of the padded quotients, records of the values vals[v k + j])"""
    zs = point_values(z_recs, layout)
    q, vals = [], []
    for c in p.vectors(data, layout, n_vec):
        qv, vv = div_points_ints(c, zs)
        q += qv
        vals += vv
    return encode(q, layout), encode(vals, layout)


def interpolate_eval(zs, ys, tau):
    """r(tau) of the polynomial of degree < k through (z_j, y_j), by Lagrange's formula"""
    acc = 0
    for j, (zj, yj) in enumerate(zip(zs, ys)):
        num = den = 1
        for m, zm in enumerate(zs):
            if m != j:
                num = num * (tau - zm) % R
                den = den * (zj - zm) % R
        acc = (acc + yj * num * pow(den, -1, R)) % R
    return acc


def vanishing_eval(zs, tau):
    acc = 1
    for z in zs:
        acc = acc * (tau - z) % R
    return acc


def same_mod_r(rec):
    """another record of the same point: its 256-bit word plus r (a reduced word is below r < 2^254)"""
    return raw([words(rec)[0] % R + R])


def point_sets(layout, k, seed):
    """(name, k records) of several sets of k pairwise distinct points: the special points of poly_ref first (as raw words
    where they have one: the words r, r + 1 and 2^256 - 1 mean what the layout makes of them), random ones to fill up;
    a set with z = 0 in it; a rotation set {z, w z, w^-1 z, ..} with w of order 2^20; random points only"""
    rng = random.Random(seed * 131 + k)

    def fresh(taken):
        while True:
            v = rng.randrange(2, R - 1)
            if v not in taken:
                return v

    sets = []
    # specials: the words r and r + 1, the residue r - 1, the word of all ones -- four distinct points in either layout
    spec = [(0, R), (1, R + 1), (R - 1, None), (((1 << 256) - 1) % R, (1 << 256) - 1)]
    rng.shuffle(spec)
    recs, taken = [], set()
    for v, w in spec[:k]:
        recs.append(p.point_record(v, layout, w))
        taken.add(decode(recs[-1], layout)[0])
    while len(recs) < k:
        v = fresh(taken)
        taken.add(v)
        recs.append(encode([v], layout))
    sets.append(("special", b"".join(recs)))
    vals = [0]
    while len(vals) < k:
        vals.append(fresh(set(vals)))
    rng.shuffle(vals)
    sets.append(("with_zero", encode(vals, layout)))
    z = rng.randrange(2, R - 1)
    rot = [z * pow(OMEGA_20, e, R) % R for e in (0, 1, -1, 2, -2, 3, -3, 4)[:k]]
    sets.append(("rotations", encode(rot, layout)))
    vals = []
    while len(vals) < k:
        vals.append(fresh(set(vals)))
    sets.append(("random", encode(vals, layout)))
    return sets
