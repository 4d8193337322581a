"""Big-integer model of the point validation (msm_amd_check_points*, msm_amd_g2_check_points*) for the tests: points
on and off the curves and the G2 subgroup, records of every host layout with the stored 256-bit integers under the
test's control (so that a coordinate >= p can be planted), and expected_reasons -- the reason code of every record from
big integers only.  g2_ref and oracle.bn254_ref are used unchanged."""
import functools
import random

import g2_ref as g
from oracle import bn254_ref as o

P, R_ORDER = o.P, o.R_ORDER
VALID, NOT_REDUCED, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(4)
CHECK_CURVE, CHECK_SUBGROUP = 1, 2
H2C, ARK_PROJECTIVE, ARK_AFFINE, JAC_BE32 = range(4)      # MSM_AMD_POINT_*
G2_H2C, G2_ARK = 0, 1                                     # MSM_AMD_G2_POINT_*
G1_BYTES = {H2C: 64, ARK_PROJECTIVE: 96, ARK_AFFINE: 72, JAC_BE32: 96}
G2_BYTES = {G2_H2C: 128, G2_ARK: 136}
X0 = 4965661367192848881                                  # the BN parameter
COFACTOR = 2 * P - R_ORDER                                # order of E'(Fq2) / r
assert P == 36 * X0**4 + 36 * X0**3 + 24 * X0**2 + 6 * X0 + 1 and R_ORDER == P - 6 * X0**2
assert COFACTOR % 10069 == 0
MAX256 = (1 << 256) - 1


# ---- Fq2 helpers ----------------------------------------------------------------------------------------------------
def pow2(a, e):
    r = g.ONE2
    while e:
        if e & 1:
            r = g.mul2(r, a)
        a = g.mul2(a, a)
        e >>= 1
    return r


def sqrt_fq(a):
    """p = 3 mod 4: a^((p + 1) / 4), None if a is no square"""
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def sqrt_fq2(a):
    """Square root in Fq2 = Fq[u] / (u^2 + 1), None if there is none: with n = sqrt(norm(a)) the root is c0 + c1 u,
    c0^2 = (a0 +- n) / 2, c1 = a1 / (2 c0)."""
    if a == g.ZERO2:
        return a
    if a[1] == 0:
        s = sqrt_fq(a[0])
        if s is not None:
            return (s, 0)
        return (0, sqrt_fq(-a[0] % P))        # -a0 is a square when a0 is not (-1 is a non-residue)
    n = sqrt_fq((a[0] * a[0] + a[1] * a[1]) % P)
    if n is None:
        return None
    half = pow(2, -1, P)
    for s in (n, -n % P):
        c0 = sqrt_fq((a[0] + s) * half % P)
        if c0:
            r = (c0, a[1] * pow(2 * c0, -1, P) % P)
            if g.mul2(r, r) == a:
                return r
    return None


XI = (9, 1)
PSI_X = pow2(XI, (P - 1) // 3)          # psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y)
PSI_Y = pow2(XI, (P - 1) // 2)


# ---- points ---------------------------------------------------------------------------------------------------------
def rand_curve_point_g2(rng):
    """A random point of the twist: random x, solved for y.  Outside G2 with overwhelming probability (asserted)."""
    while True:
        x = g.rand_fq2(rng)
        y = sqrt_fq2(g.add2(g.mul2(g.mul2(x, x), x), g.B_TWIST))
        if y is not None:
            pt = (x, y)
            assert g.on_curve(pt) and g.scalar_mul(R_ORDER, pt) is not None
            return pt


@functools.lru_cache(maxsize=None)
def special_g2(seed=1):
    """the named G2 test points, computed once: a curve point outside G2, a point of the cofactor group, a G2 point plus a
    cofactor point, a point of order 10069"""
    rng = random.Random(seed)
    q = rand_curve_point_g2(rng)
    cof = g.scalar_mul(R_ORDER, q)
    small = None
    while small is None:
        small = g.scalar_mul(R_ORDER * (COFACTOR // 10069), rand_curve_point_g2(rng))
    assert g.scalar_mul(10069, small) is None
    return {"curve": q, "cofactor": cof, "g2_plus_cofactor": g.add(g.scalar_mul(424242, g.GEN2), cof),
            "order_10069": small}


def g1_points(n, seed):
    """n valid G1 points: a progression a0 G + i d G"""
    rng = random.Random(seed)
    cur, step = o.scalar_mul(rng.randrange(1, R_ORDER), o.GEN), o.scalar_mul(rng.randrange(1, R_ORDER), o.GEN)
    out = []
    for _ in range(n):
        out.append(cur)
        cur = o.aff_add(cur, step)
    return out


def g2_points(n, seed):
    rng = random.Random(seed)
    cur, step = g.scalar_mul(rng.randrange(1, R_ORDER), g.GEN2), g.scalar_mul(rng.randrange(1, R_ORDER), g.GEN2)
    out = []
    for _ in range(n):
        out.append(cur)
        cur = g.add(cur, step)
    return out


# ---- records: the stored integers of one point in one layout ----------------------------------------------------------
class Rec:
    """coords: the stored 256-bit integers (Montgomery residues, or whatever a test plants) -- G1: x, y[, z];
    G2: x.c0, x.c1, y.c0, y.c1.  flag: the infinity byte of the ark affine layouts."""

    def __init__(self, group, layout, coords, flag=0):
        self.group, self.layout, self.coords, self.flag = group, layout, list(coords), flag

    def with_coord(self, k, v):
        c = list(self.coords)
        c[k] = v
        return Rec(self.group, self.layout, c, self.flag)

    def encode(self) -> bytes:
        if self.group == 1 and self.layout == JAC_BE32:      # 8 x u32 most significant first, host-order words
            be = b"".join(c.to_bytes(32, "big") for c in self.coords)
            return b"".join(be[4 * i:4 * i + 4][::-1] for i in range(len(be) // 4))
        body = b"".join(c.to_bytes(32, "little") for c in self.coords)
        if (self.group, self.layout) in ((1, ARK_AFFINE), (2, G2_ARK)):
            body += bytes([self.flag]) + bytes(7)
        return body


def g1_rec(layout, pt, z=1):
    """record of the affine G1 point pt (None = identity); Jacobian layouts: (x z^2, y z^3, z)"""
    m = o.fq_to_mont
    if layout in (ARK_PROJECTIVE, JAC_BE32):
        if pt is None:
            return Rec(1, layout, [m(1), m(1), 0])
        return Rec(1, layout, [m(pt[0] * z * z % P), m(pt[1] * z**3 % P), m(z % P)])
    if pt is None:
        return Rec(1, layout, [0, 0], flag=1 if layout == ARK_AFFINE else 0)
    return Rec(1, layout, [m(pt[0]), m(pt[1])])


def g2_rec(layout, pt):
    m = o.fq_to_mont
    if pt is None:
        return Rec(2, layout, [0, 0, 0, 0], flag=1 if layout == G2_ARK else 0)
    return Rec(2, layout, [m(pt[0][0]), m(pt[0][1]), m(pt[1][0]), m(pt[1][1])])


def non_reduced(rec, k, top=False):
    """coordinate k replaced by the same residue + p (still below 2^256), or by 2^256 - 1"""
    v = MAX256 if top else rec.coords[k] + P
    assert P <= v <= MAX256
    return rec.with_coord(k, v)


def encode_all(recs) -> bytes:
    return b"".join(r.encode() for r in recs)


# ---- the rule -------------------------------------------------------------------------------------------------------
def expected_reason(rec, checks):
    assert checks in (1, 2, 3)
    affine_ark = (rec.group, rec.layout) in ((1, ARK_AFFINE), (2, G2_ARK))
    if affine_ark and rec.flag:
        return VALID
    if any(c >= P for c in rec.coords):
        return NOT_REDUCED
    v = [o.fq_from_mont(c) for c in rec.coords]
    if rec.group == 1:
        if rec.layout in (ARK_PROJECTIVE, JAC_BE32):
            x, y, z = v
            if z == 0:
                return VALID
            return VALID if (y * y - x * x * x - 3 * pow(z, 6, P)) % P == 0 else NOT_ON_CURVE
        x, y = v
        if rec.layout == H2C and x == 0 and y == 0:
            return VALID
        return VALID if (y * y - x * x * x - 3) % P == 0 else NOT_ON_CURVE
    if rec.layout == G2_H2C and not any(v):
        return VALID
    pt = ((v[0], v[1]), (v[2], v[3]))
    if not g.on_curve(pt):
        return NOT_ON_CURVE
    if (checks & CHECK_SUBGROUP) and g.scalar_mul(R_ORDER, pt) is not None:
        return NOT_IN_SUBGROUP
    return VALID


def expected_reasons(recs, checks) -> bytes:
    return bytes(expected_reason(r, checks) for r in recs)


def is_identity(rec):
    """valid as an identity encoding (what n_identity counts)"""
    if (rec.group, rec.layout) in ((1, ARK_AFFINE), (2, G2_ARK)):
        return bool(rec.flag)
    if any(c >= P for c in rec.coords):
        return False
    if rec.group == 1 and rec.layout in (ARK_PROJECTIVE, JAC_BE32):
        return rec.coords[2] == 0
    return not any(rec.coords)


def expected_report(recs, checks):
    reasons = expected_reasons(recs, checks)
    bad = [i for i, r in enumerate(reasons) if r]
    return {"n_checked": len(recs), "n_invalid": len(bad), "n_identity": sum(is_identity(r) for r in recs),
            "first_invalid": bad[0] if bad else None, "first_reason": reasons[bad[0]] if bad else 0,
            "by_reason": [reasons.count(k) for k in range(4)]}, reasons


def same_report(got, want):
    return {k: got[k] for k in want} == want


# ---- planted cases ----------------------------------------------------------------------------------------------------
def g1_case_records(layout, seed):
    """(records, names): the planted G1 cases of one layout, each record at a known index"""
    rng = random.Random(seed)
    pts = g1_points(4, seed)
    jac = layout in (ARK_PROJECTIVE, JAC_BE32)
    zs = [rng.randrange(2, P) for _ in range(4)] if jac else [1] * 4
    good = [g1_rec(layout, p, z) for p, z in zip(pts, zs)]
    garbage = [rng.randrange(P, 1 << 256) for _ in range(3)]
    cases = [("valid", good[0]), ("generator", g1_rec(layout, o.GEN)), ("-generator", g1_rec(layout, o.aff_neg(o.GEN))),
             ("y + 1", good[1].with_coord(1, (good[1].coords[1] + 1) % P)),
             ("x and y swapped", good[2].with_coord(0, good[2].coords[1]).with_coord(1, good[2].coords[0])),
             ("identity", g1_rec(layout, None))]
    for k in range(len(good[3].coords)):
        cases.append((f"coordinate {k} + p", non_reduced(good[3], k)))
        cases.append((f"coordinate {k} = 2^256 - 1", non_reduced(good[3], k, top=True)))
    if layout == ARK_AFFINE:
        cases.append(("flagged, garbage coordinates", Rec(1, layout, garbage[:2], flag=1)))
        cases.append(("flag byte 0xFF", Rec(1, layout, good[0].coords, flag=0xFF)))
        cases.append(("(0, 0) without the flag", Rec(1, layout, [0, 0], flag=0)))
    if jac:
        cases.append(("random Z", g1_rec(layout, pts[1], rng.randrange(2, P))))
        cases.append(("Z = 0, any reduced X, Y", Rec(1, layout, [rng.randrange(P), rng.randrange(P), 0])))
        cases.append(("Z = 0, X not reduced", Rec(1, layout, [garbage[0], 5, 0])))
        cases.append(("good x, y with a wrong Z", good[0].with_coord(2, (good[0].coords[2] + 1) % P)))
    return [c[1] for c in cases], [c[0] for c in cases]


def g2_case_records(layout, seed):
    rng = random.Random(seed)
    pts = g2_points(4, seed)
    good = [g2_rec(layout, p) for p in pts]
    sp = special_g2()
    garbage = [rng.randrange(P, 1 << 256) for _ in range(4)]
    c = good[2].coords
    cases = [("valid", good[0]), ("EIP-197 generator", g2_rec(layout, g.GEN2)), ("-generator", g2_rec(layout, g.neg(g.GEN2))),
             ("y.c0 + 1", good[1].with_coord(2, (good[1].coords[2] + 1) % P)),
             ("y.c1 + 1", good[1].with_coord(3, (good[1].coords[3] + 1) % P)),
             ("x and y swapped", Rec(2, layout, [c[2], c[3], c[0], c[1]])),
             ("identity", g2_rec(layout, None)),
             ("curve point outside G2", g2_rec(layout, sp["curve"])),
             ("cofactor point", g2_rec(layout, sp["cofactor"])),
             ("G2 point + cofactor point", g2_rec(layout, sp["g2_plus_cofactor"])),
             ("point of order 10069", g2_rec(layout, sp["order_10069"])),
             ("-(point of order 10069)", g2_rec(layout, g.neg(sp["order_10069"])))]
    for k in range(4):
        cases.append((f"coordinate {k} + p", non_reduced(good[3], k)))
        cases.append((f"coordinate {k} = 2^256 - 1", non_reduced(good[3], k, top=True)))
    if layout == G2_ARK:
        cases.append(("flagged, garbage coordinates", Rec(2, layout, garbage, flag=1)))
        cases.append(("all zero without the flag", Rec(2, layout, [0, 0, 0, 0], flag=0)))
    return [x[1] for x in cases], [x[0] for x in cases]
