#!/usr/bin/env python3
"""Value bounds of the G2 arithmetic (bn254_fq2_29.hip.h, bn254_ec2_29.hip.h) by interval arithmetic, in multiples of
p per Fq2 component.  Every operation mirrors the code: which operand a multiplication negates through the 32 p lift,
which lifted constant each subtraction uses, where X3 and the doubling are squashed.  Iterates the point invariant to
its fixed point under madd, mmadd, the full addition and the doubling, and asserts
  * every subtrahend is below the lift of its subtraction (sub<K>: b < K p; mul / sqr: b1 / a1 < 32 p),
  * every multiplication operand is below 64 p (limb 8 < 2^28 after norm(): the 64-bit column sums then hold),
  * the zero filters' operand P stays below kG2ZeroFilter = 16 p,
  * the inversion (Fq2::inv_fq: the square-and-multiply chain over p - 2, Fq2::inv on top of norm_fq) keeps its running
    power a valid operand and meets the output bounds the headers state, and pt2_to_affine of any point inside the
    invariant yields coordinates below 2 p (what Fq29::pack_canonical, one conditional subtraction, takes).
The subgroup test of the point validation (check_points.hip.h) is part of the fixed point: psi (conjugation through the
32 p / 4 p lifts, the products by gx, gy, the squashed ZZ, ZZZ), the negation of a point, the ladder's base (canonicalised
like a stored base) and the final comparison D = L + (-R) by the full addition all stay inside the same invariant; the
curve equation's subtrahend stays below its 8 p lift.
The square roots of the decompression kernels (compress_points.hip.h) are re-derived too: the 2-bit-window ladder over
(p + 1) / 4 (every operand of a multiplication a valid one, the result below 1.05 p for an operand below 8 p), the
acceptance test through the 8 p lift, the Fq2 root (norm, halving, the negation through the 4 p lift, the inversion of
2 c, the final comparison through Fq2::sub<8>), the sign selection (canonical integer, the negated root squashed) and
the right-hand sides x^3 + b the two decoders feed in.
The batch scalar multiplication (mul_points.hip.h) adds no new point operation -- its ladder is doublings and mixed
additions of carried points with a canonical base or its 4 p negation, its digit walk mixed additions alone, both inside
the fixed point -- but a new normalisation: the shared inversion over kMulNormGroup records (prefix products of
ZZ ZZZ with the identity's substitute one, Fq2::inv of the last prefix, the backward pass) and the numerators X ZZZ and
ZZ Y; the affine coordinates it hands to aff2_pack / to_ext stay below 2 p.
Prints the invariant and the intermediate bounds; exit status 1 if an assertion fails."""
import sys

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
RP = P / 2 ** 261          # rho' = p / rho
# a reduction's result is below s / rho + ONE p: the low quotient digits of Fq29::reduce_columns reduce with a multiple of p
# and overshoot the canonical quotient by less than 2^-27 rho (masked digits, the only ones G2 uses; tools/fq29_bounds.py
# derives the figure and checks the 64-bit columns of a double product of four normalised operands)
ONE = 1 + 2.0 ** -27
LIMIT = 64                 # normalised operand value bound
ZERO_FILTER = 16
# the point invariant bn254_ec2_29.hip.h states (per component, multiples of p); main() proves the fixed point below it,
# tests/g2_stage_ref.py builds records at its edge from it
INV = {"X": 1.21, "Y": 13.4, "ZZ": 3.2, "ZZZ": 2.04}
# what the header of mul_points.hip.h states for the shared inversion of G2 (maxima over c0 and c1): MUL_NORM on the
# points the additions produce (the fixed point below, c0 and c1 carried apart), MUL_NORM_AT_INV on ANY record whose
# eight components all sit at the stated invariant at once -- coarser, and what a record written by hand may reach
# (tests/mul_stage_ref.py).  a, ZZ Y and y are the three figures that differ.
MUL_NORM = {"a": 1.29, "pre": 1.21, "inv": 1.24, "t": 1.24, "X*ZZZ": 1.25, "ZZ*Y": 1.51, "x": 1.21, "y": 1.27}
MUL_NORM_AT_INV = {"a": 1.65, "pre": 1.21, "inv": 1.24, "t": 1.24, "X*ZZZ": 1.25, "ZZ*Y": 1.86, "x": 1.21, "y": 1.30}


def chk(a):
    assert max(a) < LIMIT, a
    return a


def mul(a, b):             # c0 = a0 b0 + a1 (32 p - b1), c1 = a0 b1 + a1 b0
    assert b[1] < 32, b
    chk(a), chk(b)
    return (ONE + RP * (a[0] * b[0] + a[1] * 32), ONE + RP * (a[0] * b[1] + a[1] * b[0]))


def sqr(a):                # c0 = (a0 + a1)(a0 - a1 + 32 p), c1 = (2 a0) a1
    assert a[1] < 32, a
    chk(a)
    return (ONE + RP * (a[0] + a[1]) * (a[0] + 32), ONE + RP * 2 * a[0] * a[1])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def sub(a, b, k):
    assert max(b) < k, (b, k)
    return (a[0] + k, a[1] + k)


def squash(a):
    chk(a)
    return (ONE + RP * a[0], ONE + RP * a[1])


SEEN = {}


def note(name, v):
    SEEN[name] = tuple(max(x, y) for x, y in zip(SEEN.get(name, (0, 0)), v))
    return v


def tail(P_, R, U1, S1, tag):
    PP = sqr(P_)
    PPP = mul(P_, PP)
    Q = mul(U1, PP)
    RR = sqr(R)
    X3 = squash(sub(RR, add(PPP, add(Q, Q)), 16))
    T = sub(Q, X3, 4)
    Y3 = sub(mul(R, T), mul(S1, PPP), 8)
    for k, v in (("PP", PP), ("PPP", PPP), ("Q", Q), ("RR", RR), ("T", T)):
        note(f"{tag}.{k}", v)
    return X3, Y3, PP, PPP


def madd(X, Y, ZZ, ZZZ, qx, qy):
    U2, S2 = mul(qx, ZZ), mul(qy, ZZZ)
    P_, R = note("madd.P", sub(U2, X, 4)), note("madd.R", sub(S2, Y, 16))
    X3, Y3, PP, PPP = tail(P_, R, X, Y, "madd")
    return X3, Y3, mul(ZZ, PP), mul(ZZZ, PPP)


def mmadd(x1, y1, x2, y2):
    P_, R = note("mmadd.P", sub(x2, x1, 4)), note("mmadd.R", sub(y2, y1, 16))
    return tail(P_, R, x1, y1, "mmadd")


def add_nz(X1, Y1, ZZ1, ZZZ1, X2, Y2, ZZ2, ZZZ2):
    U1, U2, S1, S2 = mul(X1, ZZ2), mul(X2, ZZ1), mul(Y1, ZZZ2), mul(Y2, ZZZ1)
    P_, R = note("add.P", sub(U2, U1, 8)), note("add.R", sub(S2, S1, 8))
    X3, Y3, PP, PPP = tail(P_, R, U1, S1, "add")
    return X3, Y3, mul(mul(ZZ1, ZZ2), PP), mul(mul(ZZZ1, ZZZ2), PPP)


def double(X1, Y1, ZZ1, ZZZ1):
    U = add(Y1, Y1)
    V = sqr(U)
    W = mul(U, V)
    S = mul(X1, V)
    XX = sqr(X1)
    M = add(XX, add(XX, XX))
    X3 = squash(sub(sqr(M), add(S, S), 32))
    T = sub(S, X3, 4)
    Y3 = squash(sub(mul(M, T), mul(W, Y1), 8))
    return X3, Y3, squash(mul(V, ZZ1)), squash(mul(W, ZZZ1))


def fe_inv(a):            # Fq2::inv_fq: r = one; per bit of p - 2 (msb first): r = r^2, then r = r a on a set bit
    assert a < 32, a
    r, worst = 1.0, 1.0
    for bit in bin(P - 2)[2:].rjust(9 * 29, "0"):   # the loop walks all 261 bit positions of the 9 limbs
        r = ONE + RP * r * r
        worst = max(worst, r)                       # the operand of the next multiplication / squaring
        if bit == "1":
            r = ONE + RP * r * a
    assert worst < 1.02 and r < 1 + 1.02 * RP * a + 1e-12, (worst, r)
    return r


def fq2_inv(a):           # conj(a) / norm_fq(a): norm_fq = mul2(a0, a0, a1, a1), then two single products
    chk(a)
    assert max(a) < 32, a
    n = ONE + RP * (a[0] * a[0] + a[1] * a[1])
    ninv = fe_inv(n)
    return (ONE + RP * a[0] * ninv, ONE + RP * 32 * ninv)


def to_affine(X, Y, ZZ, ZZZ):   # t = (ZZ ZZZ)^-1, x = (X t) ZZZ, y = (Y t) ZZ
    t = note("affine.t", fq2_inv(note("affine.ZZ*ZZZ", mul(ZZ, ZZZ))))
    x = mul(note("affine.Xt", mul(X, t)), ZZZ)
    y = mul(note("affine.Yt", mul(Y, t)), ZZ)
    return note("affine.x", x), note("affine.y", y)


# ---- point validation (check_points.hip.h) --------------------------------------------------------------------------
def conj(a, k):           # (a0, k p - a1): the lift must cover a1; the result is anything up to k p
    assert a[1] < k, (a, k)
    return (a[0], k)


def mul_const(c, b):      # Fq2::mul(c, b) with b = conj(., 32): b1 <= 32 p (2 kc(K16E30) - b1 stays positive limb-wise)
    assert b[1] <= 32, b
    chk(c), chk((b[0], 0))
    return (ONE + RP * (c[0] * b[0] + c[1] * 32), ONE + RP * (c[0] * b[1] + c[1] * b[0]))


def psi(X, Y, ZZ, ZZZ):   # pt2_psi: (gx conj(X), gy conj(Y), squash(conj(ZZ)), squash(conj(ZZZ))), gx, gy canonical
    const = (1, 1)
    return (note("psi.X", mul_const(const, conj(X, 32))), note("psi.Y", mul_const(const, conj(Y, 32))),
            note("psi.ZZ", squash(conj(ZZ, 4))), note("psi.ZZZ", squash(conj(ZZZ, 4))))


def neg_pt(X, Y, ZZ, ZZZ):   # pt2_neg: Y' = squash(32 p - Y)
    assert max(Y) < 32, Y
    return X, note("neg.Y", squash((32, 32))), ZZ, ZZZ


def curve_equation():     # y^2 - (x^3 + b') + 8 p with x, y from_ext outputs (< 1.01 p), b' canonical
    x = y = (1.01, 1.01)
    t = note("curve.x^3", mul(sqr(x), x))
    d = note("curve.d", sub(sqr(y), add(t, (1, 1)), 8))
    chk(d)                # is_zero_exact: a multiplication operand
    # G1 (Fq29 single products): x^3 < 1 + rho' 1.01 (1 + rho' 1.01^2), Jacobian b = 3 Z^6 < 3.1 p, subtrahend < 4.2 p
    z2 = ONE + RP * 1.01 * 1.01
    z6 = ONE + RP * (ONE + RP * z2 * z2) * z2
    assert (ONE + RP * 1.01 * z2) + 3 * z6 < 8
    return d


# ---- square roots (compress_points.hip.h) -----------------------------------------------------------------------------
def fe_sqrt(a):           # comp_sqrt_candidate: table a, a^2, a^3; per 2-bit window (msb first): r = (r^2)^2, r = r a^w
    assert a < 8, a       # the contract; the acceptance test subtracts a through the 8 p lift
    a2 = ONE + RP * a * a
    a3 = ONE + RP * a2 * a
    table = {1: a, 2: a2, 3: a3}
    e = (P + 1) // 4
    r, worst, products = 1.0, 1.0, 0
    for b in range(254, -1, -2):
        r = ONE + RP * r * r
        r = ONE + RP * r * r
        worst = max(worst, r)
        w = (e >> b) & 3
        if w:
            r = ONE + RP * r * table[w]
            products += 1
            worst = max(worst, r)
    assert products == 88 and worst < 1.05 and max(a2, a3) < 1.38, (products, worst, a2, a3)
    d = (ONE + RP * r * r) + 8          # r^2 - a + 8 p: normalised, the operand of is_zero_exact
    assert d < 9.02 and ONE + RP * d < 2, d
    return r


def fq2_sqrt(a):          # comp_sqrt_fq2: a = (a0, a1), components normalised, < 4 p
    assert max(a) < 4, a
    n = ONE + RP * (a[0] * a[0] + a[1] * a[1])                # norm_fq: mul2(a0, a0, a1, a1)
    r1 = fe_sqrt(max(a[0], n))                             # in1 = a1 == 0 ? a0 : norm
    half = ONE + RP * (a[0] + r1) * 1                        # (a0 + r1) (rho / 2 mod p) / rho
    r2 = fe_sqrt(max(4.0, half))                           # in2 = a1 == 0 ? 4 p - a0 : half
    inv = fe_inv(2 * r2)                                   # inv_fq(norm(r2 + r2))
    w = ONE + RP * a[1] * inv
    root = (max(r1, r2, w), max(r2, w))
    d = sub(sqr(root), a, 8)                               # root^2 - a through Fq2::sub<8>
    chk(d)
    note("sqrt.norm", (n, n)), note("sqrt.half", (half, half)), note("sqrt.w", (w, w)), note("sqrt.root", root)
    assert n < 1.19 and half < 1.03 and w < 1.03 and max(root) < 1.05, (n, half, w, root)
    return root


def decompress():         # the two decoders: x from the canonical integer, the right-hand side, the sign selection
    x = ONE + RP * 6 * 1                                     # mul(unpack256(x < 2^254 < 6 p), rho^2 mod p)
    rhs1 = (ONE + RP * (ONE + RP * x * x) * x) + 1             # x^3 + b, b canonical
    y = fe_sqrt(rhs1)
    neg = ONE + RP * 4 * 1                                   # squash(neg(y)): neg < 4 p needs y < 3.9 p
    assert rhs1 < 2.02 and y < 3.9 and neg < 1.03 and max(x, y, neg) < 2    # packers take values below 2 p
    t = mul(sqr((x, x)), (x, x))
    rhs2 = add(t, (1, 1))
    assert max(rhs2) < 2.21, rhs2
    y2 = fq2_sqrt(rhs2)
    assert max(y2) < 2
    note("decompress.rhs", rhs2)
    lifted = fe_sqrt(8 - 1e-9)                             # the raw-limb op at the edge of its contract
    assert lifted < 1.05


# ---- batch scalar multiplication (mul_points.hip.h) -------------------------------------------------------------------
def mul_normalise(X, Y, ZZ, ZZZ, group=16, limits=None):
    """mul_normalise<MulG2> on `group` records of the invariant; an identity record contributes a = one = (rho mod p, 0)"""
    limits = limits or MUL_NORM
    one = (1.0, 0.0)
    a = note("norm.a", tuple(max(u, v) for u, v in zip(mul(ZZ, ZZZ), one)))
    xn, yn = note("norm.X*ZZZ", mul(X, ZZZ)), note("norm.ZZ*Y", mul(ZZ, Y))     # Y second: the 32 p lift multiplies ZZ
    pre, worst = one, one
    for _ in range(group):                                 # pre_i = pre_(i-1) a_i; every prefix is an operand later
        pre = mul(pre, a)
        worst = tuple(max(u, v) for u, v in zip(worst, pre))
    note("norm.pre", worst)
    inv = fq2_inv(worst)
    t_worst = (0.0, 0.0)
    for _ in range(group):                                 # t_i = inv pre_(i-1), inv = inv a_i
        t = mul(inv, worst)
        inv = tuple(max(u, v) for u, v in zip(inv, mul(inv, a)))
        t_worst = tuple(max(u, v) for u, v in zip(t_worst, t))
    note("norm.t", t_worst), note("norm.inv", inv)
    x, y = note("norm.x", mul(xn, t_worst)), note("norm.y", mul(yn, t_worst))
    for name, v in (("a", a), ("pre", worst), ("t", t_worst), ("inv", inv), ("X*ZZZ", xn), ("ZZ*Y", yn), ("x", x), ("y", y)):
        assert max(v) < limits[name], (name, v)
    assert max(x) < 2 and max(y) < 2                       # what Fq29::pack_canonical / to_ext canonicalise
    return x, y


def widen(a, b):
    return tuple(tuple(max(x, y) for x, y in zip(u, v)) for u, v in zip(a, b))


def main():
    base_x, base_y = (1, 1), (4, 4)        # canonical x; y canonical or its 4 p negation
    pt = ((1, 1), (1, 1), (1, 1), (1, 1))  # X, Y, ZZ, ZZZ
    for _ in range(20):
        new = widen(pt, madd(*pt, base_x, base_y))
        new = widen(new, mmadd(base_x, base_y, base_x, base_y))
        new = widen(new, add_nz(*new, *new))
        new = widen(new, double(*new))
        new = widen(new, double(base_x, base_y, (1, 1), (1, 1)))
        new = widen(new, psi(*new))                    # the subgroup test: psi of a carried point, ...
        new = widen(new, neg_pt(*psi(*new)))           # ... its negation, ...
        new = widen(new, add_nz(*new, *neg_pt(*new)))  # ... and the final comparison L + (-R)
        if new == pt:
            break
        pt = new
    else:
        raise AssertionError("no fixed point")
    for name in ("madd.P", "mmadd.P", "add.P"):
        assert max(SEEN[name]) < ZERO_FILTER, (name, SEEN[name])
    claimed = INV
    for (name, lim), v in zip(claimed.items(), pt):
        assert max(v) < lim, (name, v, lim)
    # the inversion at the edge of its stated input bound, and the to-affine step of the table build on any carried point
    edge = fq2_inv((32 - 1e-9, 32 - 1e-9))
    assert max(edge) < 1.21, edge
    note("inv(32p)", edge)
    x, y = to_affine(*pt)
    assert max(x) < 1.25 and max(y) < 1.3 and max(SEEN["affine.t"]) < 1.2, (x, y)
    assert max(SEEN["affine.ZZ*ZZZ"]) < 1.7 and max(SEEN["affine.Xt"]) < 1.24 and max(SEEN["affine.Yt"]) < 3.7
    assert max(SEEN["psi.X"]) < 1.21 and max(SEEN["psi.Y"]) < 1.3 and max(SEEN["psi.ZZ"]) < 1.03 and max(SEEN["neg.Y"]) < 1.2
    assert max(curve_equation()) < 9.5
    decompress()
    mul_normalise(*pt)
    seen = dict(SEEN)                      # (the printout below keeps the figures of the fixed point)
    mul_normalise(*(((v, v)) for v in INV.values()), limits=MUL_NORM_AT_INV)
    SEEN.clear()
    SEEN.update(seen)
    fq2_sqrt((4 - 1e-9, 4 - 1e-9))         # the raw-limb Fq2 root at the edge of its contract
    print("invariant: " + "  ".join(f"{k} < {max(v):.3f} p" for k, v in zip(claimed, pt)))
    for k in sorted(SEEN):
        print(f"  {k:10s} < {max(SEEN[k]):.2f} p")
    return 0


if __name__ == "__main__":
    sys.exit(main())
