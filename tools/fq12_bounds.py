"""Re-derives the figures of the bounds contract of csrc/bn254_fq12_29.hip.h (multiples of p per Fq component), in the
manner of tools/g2_bounds.py: every function of the header is replayed on upper bounds, with the output rules of
bn254_fq29.hip.h / bn254_fq2_29.hip.h:

  a reduction of accumulated limb-product sets sum_t x_t y_t        : value < (1 + rho' sum X_t Y_t) p,  rho' = p / 2^261
  Fq2::mul(a, b) = (a0 b0 + a1 (32 p - b1),  a0 b1 + a1 b0)          : b1 < 32 p
  Fq2::sqr(a)    = ((a0 + a1)(a0 - a1 + 32 p),  (2 a0) a1)
  sub<K>(a, b)   = a - b + K p, b < K p;  add, k a: sums;  squash(a) = a * 1

and checks the operand conditions on the way (second operands of an accumulated product below 8 p, sub<K> operands
below K p, every multiplication operand below 32 p, the 64-bit columns).

  python3 tools/fq12_bounds.py                 prints every figure
  python3 tools/fq12_bounds.py --check-header  also checks that the header quotes each of them
"""
import math
import os
import sys

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
RHOP = P / 2.0**261
ELEMENT = 4.0       # every component of an fq12 / fq6 the functions take and return
SECOND = 8.0        # bound of the negated imaginary part 8 p - b1 of a second operand
FIG = {}


def red(sets):
    """one reduction over limb-product sets [(X, Y), ...]; at most six sets share the columns"""
    assert len(sets) <= 6, "more than six sets in one reduction"
    return 1 + RHOP * sum(x * y for x, y in sets)


class F2:
    """upper bounds of the two components of an Fq2"""

    def __init__(self, c0, c1=None):
        self.c0, self.c1 = c0, c0 if c1 is None else c1

    def max(self):
        return max(self.c0, self.c1)


def mul(a, b):
    assert b.c1 < 32 and a.max() < 40 and b.max() < 40
    return F2(red([(a.c0, b.c0), (a.c1, 32)]), red([(a.c0, b.c1), (a.c1, b.c0)]))


def sqr(a):
    assert a.c1 < 32 and a.c0 + a.c1 < 40
    return F2(red([(a.c0 + a.c1, a.c0 + 32)]), red([(2 * a.c0, a.c1)]))


def sub(k, a, b):
    assert b.max() < k, ("sub<%d> operand" % k, b.max())
    return F2(a.c0 + k, a.c1 + k)


def add(a, b):
    return F2(a.c0 + b.c0, a.c1 + b.c1)


def times(a, k):
    assert k <= 7
    return F2(a.c0 * k, a.c1 * k)


def squash(a):
    assert a.max() < 40
    return F2(red([(a.c0, 1)]), red([(a.c1, 1)]))


def scale(a, s):
    assert a.max() < 40 and s < 40
    return F2(red([(a.c0, s)]), red([(a.c1, s)]))


def acc(products, scaled=()):
    """accumulated Fq2 products [(a, b), ...] (+ a s for Fq s), one reduction per component: b < 8 p, b1 negated to 8 p"""
    re_sets, im_sets = [], []
    for a, b in products:
        assert b.max() < SECOND + 1e-9, ("second operand", b.max())
        re_sets += [(a.c0, b.c0), (a.c1, SECOND)]
        im_sets += [(a.c0, b.c1), (a.c1, b.c0)]
    for a, s in scaled:
        re_sets.append((a.c0, s))
        im_sets.append((a.c1, s))
    return F2(red(re_sets), red(im_sets))


CONST = F2(1.0)                      # xi, 3 b', gamma: canonical


def mul_xi(b):
    return mul(CONST, b)


def derive():
    E = F2(ELEMENT)
    # the 64-bit columns of six sets of normalised limbs plus the nine terms of a masked quotient digit
    col = 54 * (2**29 + 8) ** 2 + 9 * 2**58
    assert col < 2**64
    FIG["columns"] = math.log2(col)
    xb = mul_xi(F2(7.99))
    FIG["xi_b"] = xb.max()
    # fq12_mul: two reductions of three products each, added; a wrapped product uses xi b (smaller than b)
    half = acc([(E, E)] * 3)
    FIG["fq12_mul"] = 2 * half.max()
    assert FIG["fq12_mul"] <= ELEMENT
    # fq12_sqr: cross terms with the first operand doubled; an even coefficient is two reductions of a doubled product and
    # a square (or of two doubled products and of two squares: the same sum), an odd one one reduction of three doubled
    E2 = times(E, 2)
    even_k = max(2 * acc([(E2, E), (E, E)]).max(), acc([(E2, E)] * 2).max() + acc([(E, E)] * 2).max())
    FIG["fq12_sqr"] = max(even_k, acc([(E2, E)] * 3).max())
    assert FIG["fq12_sqr"] <= ELEMENT
    FIG["fq6_mul"] = acc([(E, E)] * 3).max()
    line = F2(SECOND - 0.01)
    FIG["fq12_mul_line"] = acc([(E, line)] * 3).max()
    # cyclotomic squaring
    xbe = mul_xi(E)
    even = acc([(times(E, 3), E), (times(xbe, 3), E)], [(E, 4.0)])
    odd = acc([(times(E, 6), E)], [(E, 2.0)])
    FIG["cyclo_even"], FIG["cyclo_odd"] = even.max(), odd.max()
    assert max(even.max(), odd.max()) <= ELEMENT
    FIG["fq12_frob"] = mul(CONST, F2(ELEMENT)).max()
    # fq6_inv on components below 8 p (fq12_inv hands it t0 - v t1 + 4 p)
    t = sub(4, F2(FIG["fq6_mul"]), F2(FIG["fq6_mul"]))
    FIG["inv_t"] = t.max()
    a = F2(t.max())
    xa = mul_xi(a)
    n8 = F2(SECOND)
    A = acc([(a, a), (n8, a)])
    B = acc([(xa, a), (n8, a)])
    F = acc([(a, A), (xa, B), (xa, A)])
    assert F.max() < 32
    fi = F2(1.21)                                   # Fq2::inv: < 1.21 p (bn254_fq2_29.hip.h)
    FIG["fq6_inv"] = max(mul(fi, A).max(), mul(fi, B).max())
    FIG["fq12_inv"] = max(acc([(E, F2(FIG["fq6_inv"]))] * 3).max(), acc([(n8, F2(FIG["fq6_inv"]))] * 3).max())
    assert FIG["fq12_inv"] <= ELEMENT
    # the steps: T at the element bound, Q.y possibly negated (4 p), P canonical
    T = F2(ELEMENT)
    b, c = sqr(T), sqr(T)
    e = mul(CONST, c)
    f = times(e, 3)
    yz = mul(T, T)
    h = add(yz, yz)
    j = sqr(T)
    xy = mul(T, T)
    e2 = sqr(add(e, e))
    s = sqr(add(b, f))
    dl0 = scale(h, 4.0)
    dl1 = scale(times(j, 3), 1.0)
    dl3 = sub(4, e, b)
    dx = mul(add(xy, xy), sub(8, b, f))
    dy = squash(sub(8, s, times(e2, 3)))
    dz = mul(add(b, b), add(h, h))
    Q = F2(1.04, 4.0)                                # x canonical; y a negation
    Qy = F2(4.0)
    theta = sub(4, T, mul(T, Qy))
    lam = sub(4, T, mul(T, F2(1.3)))
    cc, d = sqr(theta), sqr(lam)
    ee = mul(lam, d)
    ff = mul(T, cc)
    g = mul(T, d)
    hh = sub(8, add(ee, ff), add(g, g))
    al0 = scale(lam, 1.0)
    al1 = scale(theta, 4.0)
    al3 = sub(4, mul(F2(1.3), theta), mul(Qy, lam))
    t1 = mul(theta, sub(16, g, hh))
    ax = mul(lam, hh)
    ay = squash(sub(4, t1, mul(ee, T)))
    az = mul(T, ee)
    FIG["step_x"] = max(dx.max(), ax.max())
    FIG["step_y"] = max(dy.max(), ay.max())
    FIG["step_z"] = max(dz.max(), az.max())
    FIG["line_l0"] = max(dl0.max(), al0.max())
    FIG["line_l1"] = max(dl1.max(), al1.max())
    FIG["line_l3"] = max(dl3.max(), al3.max())
    assert max(FIG["step_x"], FIG["step_y"], FIG["step_z"]) <= ELEMENT and FIG["line_l3"] < SECOND
    assert Q.max() <= ELEMENT


def quoted(key):
    v = FIG[key]
    return ("2^%.2f" % (math.ceil(v * 100) / 100)) if key == "columns" else ("%.2f p" % (math.ceil(v * 100) / 100))


def main():
    derive()
    for k in FIG:
        print("%-14s %s" % (k, quoted(k)))
    if "--check-header" in sys.argv:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        hdr = open(os.path.join(root, "metal-msm-gpu-acceleration_amd", "csrc", "bn254_fq12_29.hip.h")).read()
        missing = [k for k in FIG if ("[%s] " % k) not in hdr or ("[%s] %s" % (k, quoted(k))) not in hdr]
        if missing:
            print("the header does not quote: " + ", ".join("[%s] %s" % (k, quoted(k)) for k in missing))
            return 1
        print("all figures of bn254_fq12_29.hip.h re-derived")
    return 0


if __name__ == "__main__":
    sys.exit(main())
