"""Worst-case limb-bound verifier for the lazily reduced 29-bit-limb arithmetic (csrc/bn254_fq29.hip.h,
bn254_ec29.hip.h).

The hot kernels never propagate carries between field operations: limbs are only BOUNDED, and a 64-bit column sum
of a multiplication that overflowed would be silent.  This script re-states the group-law formulas over intervals
(per-limb maxima, value bound in multiples of p) and checks, for every multiplication, squaring and double
product, that no column of products + Montgomery terms + carries (+ the additive tail K - x where the lifted subtraction
is folded into the reduction: mul_sub_np / sqr_sub_np) can reach 2^64, that no lifted subtraction can go negative in any limb, that no limb leaves 32 bits, that the one-limb zero filters are given a large enough
bound, and that every point an addition returns satisfies the invariant the next addition assumes
(X < 10 p, Y < 6 p, ZZ < 2.8 p, ZZZ < 2 p, limbs 0..7 < 2^29 + 8).  Run: python tools/fq29_bounds.py  (exit 0 = all hold).
The constants are read from the header, the formulas below mirror bn254_ec29.hip.h line by line -- when one
changes, change the other."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc", "bn254_fq29.hip.h")
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
MASK = (1 << 29) - 1
RHO = 1 << 261
src = open(HDR).read()


def _table(name, rows=1):
    m = re.search(name + r"\(int[^)]*\)\s*\{\s*constexpr uint32_t c(?:\[\d+\])?\[9\] = \{(.*?)\};", src, re.S)
    nums = [int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]+)u", m.group(1))]
    return [nums[9 * r:9 * r + 9] for r in range(len(nums) // 9)]


PL = _table("p")[0]
assert sum(l << (29 * i) for i, l in enumerate(PL)) == P
KC = _table("kc")
KNAMES = ["K4E30", "K8E30", "K8E31", "K16E30", "K16E31", "K12E30"]
KMULT = {}
for name, limbs in zip(KNAMES, KC):
    v = sum(l << (29 * i) for i, l in enumerate(limbs))
    assert v % P == 0
    KMULT[name] = v // P
KL = dict(zip(KNAMES, KC))
problems = []


def fail(msg):
    problems.append(msg)


class Fe:
    """limb maxima (limbs are unsigned, minima are 0) + value bound in multiples of p"""

    def __init__(self, mx, val, name="?"):
        self.mx, self.val, self.name = list(mx), float(val), name

    def __repr__(self):
        return f"{self.name}: val<{self.val:.2f}p, limbs<=2^{max(self.mx[:8]).bit_length()} top<={self.mx[8]}"


def top_from_value(val):
    return int(val * P) >> 232


def canonical(name):          # an unpacked base coordinate: canonical limbs of a value < p
    return Fe([MASK] * 8 + [P >> 232], 1.0, name)


# reduce_columns: digits 0..6 reduce with N = INVF p = 2^29 NPP - 1 (the digit is the column's own low 29 bits, or its
# low 32 bits when WIDE; the products digit * NPP_j go to columns k + 1 .. k + 9; the rest of the column is the carry),
# digits 7 and 8 are the classic A[k] * INV (digit 7 keeps 32 bits when WIDE, digit 8 its mask).
NPP = _table("npp")[0]
INV29 = int(re.search(r"INV = 0x([0-9A-Fa-f]+)u", src).group(1), 16)
FRIENDLY_DIGITS = int(re.search(r"FRIENDLY_DIGITS = (\d+);", src).group(1))
assert (INV29 * P + 1) % (1 << 29) == 0
_N = (sum(l << (29 * i) for i, l in enumerate(NPP)) << 29) - 1
assert _N % P == 0 and (_N // P) % (1 << 29) == INV29, "npp is not (INVF p + 1) / 2^29 with INVF = INV mod 2^29"
INVF = _N // P
DIGIT_MAX = {False: [MASK] * 9, True: [(1 << 32) - 1] * 8 + [MASK]}


def quotient_excess(wide):
    """The digits add up to Q = Q0 (mod rho), Q0 < rho the canonical quotient, and Q = T + digit_8 2^232 with T the sum
    of digits 0..7 at their weights: Q is Q0, or Q0 + rho when Q0 < T.  Returns the largest T over rho: the result is
    below s / rho + p (1 + that), and it is mont(s) + p only for products whose Q0 is below T."""
    d = DIGIT_MAX[wide]
    t = sum(d[k] * INVF << (29 * k) for k in range(FRIENDLY_DIGITS)) + sum(d[k] << (29 * k) for k in range(FRIENDLY_DIGITS, 8))
    assert t < RHO
    return t / RHO


EXTRA = {w: quotient_excess(w) * 1.001 for w in (False, True)}
assert EXTRA[True] < 2.0 ** -24 and EXTRA[False] < 2.0 ** -27, EXTRA
WIDE_EXTRA = EXTRA[True]


def _reduce(cols, what, wide=False, tail=None):
    """Montgomery reduction of worst-case column sums (every step is monotone in the columns, so every digit and every
    carry at its maximum bounds them all); returns the worst-case top limb (final carry).  tail: the limb maxima of
    reduce_columns' additive tail; limbs 0..7 join columns 9..16 in front of the output carry chain."""
    A = list(cols) + [0] * (17 - len(cols))
    carry = 0
    for k in range(9):
        if k < FRIENDLY_DIGITS:
            if A[k] >= 1 << 64:
                fail(f"{what}: column {k} can reach 2^{A[k].bit_length()} during the reduction")
            for j in range(9):
                A[k + 1 + j] += DIGIT_MAX[wide][k] * NPP[j]
            A[k + 1] += (A[k] >> 32) * 8 if wide else A[k] >> 29
            continue
        A[k] += carry
        for j in range(9):
            A[k + j] += DIGIT_MAX[wide][k] * PL[j]
        if A[k] >= 1 << 64:
            fail(f"{what}: column {k} can reach 2^{A[k].bit_length()} during the reduction")
        carry = A[k] >> 29
    if tail is not None:
        for k in range(9, 17):
            A[k] += tail[k - 9]
    for k in range(9, 17):
        A[k] += carry
        if A[k] >= 1 << 64:
            fail(f"{what}: column {k} can reach 2^{A[k].bit_length()}")
        carry = A[k] >> 29
    return carry


def _mul_cols(pairs):
    cols = [0] * 17
    for a, b in pairs:
        for i in range(9):
            for j in range(9):
                cols[i + j] += a.mx[i] * b.mx[j]
    return cols


def _out(pairs, name, what, wide=False):
    for a, b in pairs:
        for f in (a, b):
            if max(f.mx) >= 1 << 32:
                fail(f"{what}: operand {f.name} has a limb beyond 32 bits")
    carry = _reduce(_mul_cols(pairs), what + (" (wide digits)" if wide else ""), wide)
    val = sum(a.val * b.val for a, b in pairs) * P / RHO + 1.0 + EXTRA[wide]
    top = min(carry, top_from_value(val))
    return Fe([MASK] * 8 + [top], val, name)


def _out_sub(pairs, sel, x, name, what):
    """The forms with the lifted subtraction folded into the reduction (Fq29::mul_sub_np, sqr_sub_np: wide digits):
    d = K - x limb by limb, x under sub<K>'s operand contract (so no limb of d goes negative and every one stays below
    2^32); d[0..7] join columns 9..16, d[8] the top limb.  Checked: the columns with the injected term (< 2^64), the
    top limb carry + K[8] - x[8] (not negative: x[8] <= K[8]; inside 32 bits).  The output carry chain leaves limbs
    0..7 below 2^29 exactly, so the top limb is also the value's own: floor(value / 2^232)."""
    K = KL[sel]
    for a, b in pairs:
        for f in (a, b):
            if max(f.mx) >= 1 << 32:
                fail(f"{what}: operand {f.name} has a limb beyond 32 bits")
    for i in range(9):
        if x.mx[i] > K[i]:
            fail(f"{what}: limb {i} of the subtrahend {x.name} may exceed the lift of {sel} ({x.mx[i]:#x} > {K[i]:#x})")
    if x.val > KMULT[sel]:
        fail(f"{what}: subtrahend value {x.val:.2f}p above the {KMULT[sel]}p of {sel}")
    d = list(K)                                  # the largest K - x: x = 0
    if max(d) >= 1 << 32:
        fail(f"{what}: a limb of {sel} - {x.name} leaves 32 bits")
    carry = _reduce(_mul_cols(pairs), what + " (wide digits, additive tail)", True, d)
    if carry + d[8] >= 1 << 32:
        fail(f"{what}: the top limb carry + K[8] - x[8] may leave 32 bits")
    val = sum(a.val * b.val for a, b in pairs) * P / RHO + 1.0 + EXTRA[True] + KMULT[sel]
    top = min(carry + d[8], top_from_value(val))
    folds.add(what)
    return Fe([MASK] * 8 + [top], val, name)


folds = set()                                    # every folded subtraction the formulas below use (main() counts them)


def mul_sub(sel, a, b, x, name):
    return _out_sub([(a, b)], sel, x, name, f"mul_sub<{sel}> {name} = {a.name} * {b.name} - {x.name}")


def sqr_sub(sel, a, x, name):
    if max(a.mx) * 2 >= 1 << 32:
        fail(f"sqr_sub {name}: doubled limb of {a.name} leaves 32 bits")
    return _out_sub([(a, a)], sel, x, name, f"sqr_sub<{sel}> {name} = {a.name}^2 - {x.name}")


# wide=True: the forms with wide quotient digits (Fq29::mul_np, sqr_np, mul2w_np; mul2_np is masked)
def mul(a, b, name, wide=False):
    return _out([(a, b)], name, f"mul {name} = {a.name} * {b.name}", wide)


def mul2(a, b, c, d, name, wide=False):
    return _out([(a, b), (c, d)], name, f"mul2 {name} = {a.name}*{b.name} + {c.name}*{d.name}", wide)


def sqr(a, name, wide=False):
    if max(a.mx) * 2 >= 1 << 32:
        fail(f"sqr {name}: doubled limb of {a.name} leaves 32 bits")
    return _out([(a, a)], name, f"sqr {name} = {a.name}^2", wide)


def add(a, b, name=None):
    r = Fe([x + y for x, y in zip(a.mx, b.mx)], a.val + b.val, name or f"({a.name}+{b.name})")
    if max(r.mx) >= 1 << 32:
        fail(f"add {r.name}: limb beyond 32 bits")
    return r


def sub(sel, a, b, name):
    K = KL[sel]
    for i in range(9):
        if b.mx[i] > K[i]:
            fail(f"sub<{sel}> {name} = {a.name} - {b.name}: limb {i} of the subtrahend may exceed the lift "
                 f"({b.mx[i]:#x} > {K[i]:#x})")
    if b.val > KMULT[sel]:
        fail(f"sub<{sel}> {name}: subtrahend value {b.val:.2f}p above the {KMULT[sel]}p of the constant")
    r = Fe([x + k for x, k in zip(a.mx, K)], a.val + KMULT[sel], name)
    if max(r.mx) >= 1 << 32:
        fail(f"sub<{sel}> {name}: limb beyond 32 bits")
    return r


def norm(a, name=None):
    mx = [min(a.mx[0], MASK)]
    for i in range(1, 8):
        mx.append(min(a.mx[i], MASK) + (a.mx[i - 1] >> 29))
    mx.append(a.mx[8] + (a.mx[7] >> 29))
    top = min(mx[8], top_from_value(a.val) + 1)
    mx[8] = top
    return Fe(mx, a.val, name or a.name)


def zero():
    return Fe([0] * 9, 0.0, "0")


def neg(a, name):
    return norm(sub("K4E30", zero(), a, name), name)


# the one-limb zero filters: the bound each site needs (the smallest integer above the value bound of its operand) and
# the constant the header gives it (kZeroFilter* in bn254_ec29.hip.h); main() prints both
EC_HDR = os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc", "bn254_ec29.hip.h")
FILTERS = {m.group(1): int(m.group(2))
           for m in re.finditer(r"constexpr uint32_t (kZeroFilter\w+) = (\d+);", open(EC_HDR).read())}
derived_filters = {}


def maybe_zero(a, site):
    need = int(a.val) + 1
    derived_filters[site] = max(need, derived_filters.get(site, 0))
    bound = FILTERS.get(site)
    if bound is None:
        fail(f"maybe_zero({a.name}, {site}): the header has no constant {site}")
    elif a.val >= bound:
        fail(f"maybe_zero({a.name}, {site} = {bound}): value bound {a.val:.2f}p is not below the filter's {bound}")


# the invariant of every stored / loop-carried point (multiples of p).  On E (packed bases) pti_mmadd sets it: ZZ3 = P^2
# with P < 17.1 p gives 2.72 p, X3 = R^2 - ... + 8 p with R < 12.1 p gives 9.86 p.  On E' (the caller's bases read in
# place: x = E << 3 < 8 p, y = E << 2 < 4 p, -y = 8 p - y) P and R of the affine start are below 24.1 p, which gives
# ZZ3 < 4.5 p and X3 < 12.5 p, and a bucket of ONE base stores x < 8 p, |y| <= 8 p as they were gathered.
class Inv:
    def __init__(self, name, x, y, zz, zzz):
        self.name, self.x, self.y, self.zz, self.zzz = name, x, y, zz, zzz


INV_E = Inv("E", 10.0, 6.0, 2.8, 2.0)
INV_ISO = Inv("E'", 11.5, 8.0, 3.4, 2.0)
INV_X, INV_Y, INV_ZZ, INV_ZZZ = INV_E.x, INV_E.y, INV_E.zz, INV_E.zzz


def check_point(x, y, zz, zzz, where, inv=INV_E):
    for f, lim in ((x, inv.x), (y, inv.y), (zz, inv.zz), (zzz, inv.zzz)):
        if f.val > lim:
            fail(f"{where}: {f.name} may reach {f.val:.2f}p, the invariant says < {lim}p")
        if max(f.mx[:8]) > MASK + 8:
            fail(f"{where}: {f.name} leaves limbs above 2^29 + 8")


def point_invariant(inv=INV_E):
    def coord(name, val):
        return Fe([MASK + 8] * 8 + [top_from_value(val) + 1], val, name)
    return coord("X1", inv.x), coord("Y1", inv.y), coord("ZZ1", inv.zz), coord("ZZZ1", inv.zzz)


# ---- the bases as the accumulate kernel sees them -----------------------------------------------------------
class Bases:
    """packed: canonical x, y < p of the internal domain (AffPacked), -y = 4 p - y.
    in place: the caller's canonical E = x R mod p sliced out of E << 3 (x) and E << 2 (y) -- Fq29::unpack256_shl -- the
    coordinates of the image on E': y'^2 = x'^3 + 3/64; exact 29-bit limbs, values < 8 p and < 4 p, -y = 8 p - y (the
    top limb of a y just below 4 p is above the borrowed top limb of K4E30)."""

    def __init__(self, iso):
        self.iso = iso
        self.inv = INV_ISO if iso else INV_E
        self.tag = " (E')" if iso else ""
        self.neg_sel = "K8E30" if iso else "K4E30"
        self.start_sel = ("K12E30", "K12E30") if iso else ("K16E30", "K8E30")   # pti_mmadd_head: P, R
        self.filter_mmadd = "kZeroFilterMmaddIso" if iso else "kZeroFilterMmadd"

    def x(self, name):
        return Fe([MASK] * 8 + [(8 * (P - 1)) >> 232], 8.0, name) if self.iso else canonical(name)

    def y(self, name):
        return Fe([MASK] * 8 + [(4 * (P - 1)) >> 232], 4.0, name) if self.iso else canonical(name)

    def negated_y(self, name="+-y2"):
        """accumulate_kernel: cur.y = negate ? -y : y  (no carry round)"""
        qy = self.y(name[2:])
        n = sub(self.neg_sel, zero(), qy, "-y")
        return Fe([max(a, b) for a, b in zip(n.mx, qy.mx)], max(n.val, qy.val), name)

    def stored_y(self, name="+-y1"):
        """pti_from_affi: the y of a point that becomes an accumulator is normalised"""
        return norm(self.negated_y(name), name)


PACKED, IN_PLACE = Bases(False), Bases(True)


# ---- the formulas of bn254_ec29.hip.h ----------------------------------------------------------------------
WD = True   # the point additions' products use wide quotient digits where the header's _np forms do
def pti_double(px, py, pzz, pzzz, where, inv=INV_E):
    U = add(py, py, "U")
    V = sqr(U, "V")
    W = mul(U, V, "W")
    S = mul(px, V, "S")
    XX = sqr(px, "XX")
    M = norm(add(XX, add(XX, XX)), "M")
    MM = sqr(M, "MM")
    X3 = norm(sub("K4E30", MM, add(S, S), "X3"), "X3")
    T = norm(sub("K8E30", S, X3, "T"), "T")
    Y3 = norm(sub("K4E30", mul(M, T, "MT"), mul(W, py, "WY"), "Y3"), "Y3")
    ZZ3 = mul(V, pzz, "ZZ3")
    ZZZ3 = mul(W, pzzz, "ZZZ3")
    check_point(X3, Y3, ZZ3, ZZZ3, where + " (doubling)", inv)


def neg_wide(a, name, sel="K4E30"):
    return sub(sel, zero(), a, name)


def negated_base_y(qy, name="+-y2"):
    """accumulate_kernel: cur.y = negate ? Fq29::neg_wide(cur.y) : cur.y  (no carry round)"""
    n = neg_wide(qy, "-y")
    return Fe([max(a, b) for a, b in zip(n.mx, qy.mx)], max(n.val, qy.val), name)


def stored_base_y(qy, name="+-y1"):
    """pti_from_affi: the y of a point that becomes an accumulator is normalised"""
    return norm(negated_base_y(qy, name), name)


def general_point(inv):
    """the accumulator of the mixed addition: a sum of at least two bases (pti_mmadd, pti_madd or pti_double output),
    whose Y is below 6 p on either curve -- only a lone base (pti_from_affi) carries the 8 p of a negated y on E'"""
    px, py, pzz, pzzz = point_invariant(inv)
    y6 = point_invariant(INV_E)[1]
    return px, y6, pzz, pzzz


def pti_madd(bases=PACKED):
    where = "pti_madd" + bases.tag
    px, py, pzz, pzzz = general_point(bases.inv)
    qx, qy = bases.x("x2"), bases.negated_y()
    U2 = mul(qx, pzz, "U2", WD)                              # the figure only: the head folds X1 and Y1 in
    Pd = mul_sub("K16E30", qx, pzz, px, "P")                 # pti_madd_head: U2 - X1, S2 - Y1 in the reductions
    R = mul_sub("K8E30", qy, pzzz, py, "R")
    maybe_zero(Pd, "kZeroFilterMadd")
    PP = sqr(Pd, "PP", WD)
    PPP = mul(Pd, PP, "PPP", WD)
    Q = mul(px, PP, "Q", WD)
    X3 = sqr_sub("K8E31", R, add(PPP, add(Q, Q)), "X3")      # R^2 - PPP - 2 Q in the reduction of R^2
    T = sub("K16E30", Q, X3, "T")                            # un-normalised: its partner R is normalised
    Y3 = mul2(R, T, py, neg_wide(PPP, "-PPP"), "Y3")          # mul2_np: masked digits
    ZZ3 = mul(pzz, PP, "ZZ3", WD)
    ZZZ3 = mul(pzzz, PPP, "ZZZ3", WD)
    check_point(X3, Y3, ZZ3, ZZZ3, where, bases.inv)
    if Y3.val > INV_E.y:
        fail(f"{where}: Y3 may reach {Y3.val:.2f}p, the accumulator of the next mixed addition is taken below {INV_E.y}p")
    one = Fe([MASK] * 8 + [P >> 232], 1.0, "one")           # the doubling path restarts from pti_from_affi(q)
    pti_double(qx, bases.stored_y(), one, one, where, INV_E)   # a doubling's outputs obey E's figures on either curve
    return {"U2": U2, "P": Pd, "R": R, "X3": X3, "Y3": Y3, "ZZ3": ZZ3, "ZZZ3": ZZZ3}


def pti_mmadd(bases=PACKED):
    # both operands affine; p = a previous base (its y possibly a lazily negated value), q likewise
    where = "pti_mmadd" + bases.tag
    px, py = bases.x("x1"), bases.stored_y()
    qx, qy = bases.x("x2"), bases.negated_y()
    Pd = norm(sub(bases.start_sel[0], qx, px, "P"), "P")
    R = norm(sub(bases.start_sel[1], qy, py, "R"), "R")
    maybe_zero(Pd, bases.filter_mmadd)
    PP = sqr(Pd, "PP", WD)
    PPP = mul(Pd, PP, "PPP", WD)
    Q = mul(px, PP, "Q", WD)
    X3 = sqr_sub("K8E31", R, add(PPP, add(Q, Q)), "X3")
    T = norm(sub("K16E30", Q, X3, "T"), "T")
    Y3 = mul2(R, T, py, neg_wide(PPP, "-PPP"), "Y3")
    check_point(X3, Y3, PP, PPP, where, bases.inv)
    if Y3.val > INV_E.y:
        fail(f"{where}: Y3 may reach {Y3.val:.2f}p, the accumulator of the next mixed addition is taken below {INV_E.y}p")
    one = Fe([MASK] * 8 + [P >> 232], 1.0, "one")
    pti_double(qx, bases.stored_y(), one, one, where, INV_E)
    return {"P": Pd, "R": R, "X3": X3, "Y3": Y3, "ZZ3": PP, "ZZZ3": PPP}


def pti_add_nz(inv=INV_E):
    """add-2008-s in 11 reductions: P and R as double products with the subtrahend negated (neg_wide), V = ZZ2 PP and
    Tz = ZZZ2 PPP shared by Q / ZZ3 and Y3 / ZZZ3.  The operands are any two points of the invariant: sums, doublings
    and, through pti_from_affi, lone bases (ZZ = ZZZ = one, inside the same figures)."""
    where = "pti_add_nz" + ("" if inv is INV_E else " (E')")
    px, py, pzz, pzzz = point_invariant(inv)
    qx, qy, qzz, qzzz = point_invariant(inv)
    for f, n in ((qx, "X2"), (qy, "Y2"), (qzz, "ZZ2"), (qzzz, "ZZZ2")):
        f.name = n
    Pd = mul2(qx, pzz, px, neg_wide(qzz, "-ZZ2"), "P", WD)
    R = mul2(qy, pzzz, py, neg_wide(qzzz, "-ZZZ2"), "R", WD)
    maybe_zero(Pd, "kZeroFilterAdd")
    PP = sqr(Pd, "PP", WD)
    PPP = mul(Pd, PP, "PPP", WD)
    V = mul(qzz, PP, "V", WD)
    Tz = mul(qzzz, PPP, "Tz", WD)
    Q = mul(px, V, "Q", WD)
    X3 = sqr_sub("K8E31", R, add(PPP, add(Q, Q)), "X3")
    T = sub("K16E30", Q, X3, "T")
    Y3 = mul2(R, T, py, neg_wide(Tz, "-Tz"), "Y3")            # mul2_np: masked digits
    ZZ3 = mul(pzz, V, "ZZ3", WD)
    ZZZ3 = mul(pzzz, Tz, "ZZZ3", WD)
    check_point(X3, Y3, ZZ3, ZZZ3, where, INV_E)    # a full addition's outputs obey E's figures on either curve
    pti_double(px, py, pzz, pzzz, where, inv)
    return {"P": Pd, "R": R, "X3": X3, "Y3": Y3, "ZZ3": ZZ3, "ZZZ3": ZZZ3}


def widen(a, b, name):
    return Fe([max(x, y) for x, y in zip(a.mx, b.mx)], max(a.val, b.val), name)


def inv_fq(a, name):
    """Fq2::inv_fq (bn254_fq2_29.hip.h): r = one; per bit of p - 2 over the 261 bit positions of the limbs, most
    significant first: r = r^2, then r = r a on a set bit"""
    r = Fe([MASK] * 8 + [P >> 232], 1.0, "one")
    for bit in bin(P - 2)[2:].rjust(261, "0"):
        r = sqr(r, "r^2")
        if bit == "1":
            r = mul(r, a, "r*a")
    r.name = name
    return r


# what the header of mul_points.hip.h states for the shared inversion (multiples of p; the figures are rounded, hence the
# slack); tests/mul_stage_ref.py checks the records mul_normalise leaves behind against the same numbers
MUL_NORM = {"a": 1.04, "pre": 1.01, "inv": 1.01, "t": 1.01, "X*ZZZ": 1.12, "ZZ*Y": 1.10, "x": 1.01, "y": 1.01}
MUL_NORM_SLACK = 0.005


def mul_points(group=16, where="mul_normalise"):
    """mul_points.hip.h.  The ladder and the digit walk are pti_double and pti_madd on points of the invariant with a
    canonical base or its normalised negation -- the cases above (pti_double is checked at the invariant inside
    pti_add_nz, the negated base inside pti_madd).  New is the shared inversion of the normalisation: a = ZZ ZZZ (one for
    an identity record), prefix products, inv_fq, the backward pass, the numerators X ZZZ and ZZ Y, and the affine
    coordinates handed to affi_pack / to_ext, which canonicalise multiplication outputs below 2 p."""
    px, py, pzz, pzzz = point_invariant()
    one = Fe([MASK] * 8 + [P >> 232], 1.0, "one")
    a = widen(mul(pzz, pzzz, "a"), one, "a")
    xn, yn = mul(px, pzzz, "X*ZZZ"), mul(pzz, py, "ZZ*Y")
    pre = one
    for _ in range(group):
        pre = widen(pre, mul(pre, a, "pre"), "pre")
    inv = inv_fq(pre, "inv")
    t = one
    for _ in range(group):
        t = widen(t, mul(inv, pre, "t"), "t")
        inv = widen(inv, mul(inv, a, "inv"), "inv")
    x, y = mul(xn, t, "x"), mul(yn, t, "y")
    for f in (a, pre, inv, t, xn, yn, x, y):
        lim = MUL_NORM[f.name]
        if f.val >= lim + MUL_NORM_SLACK:
            fail(f"{where}: {f.name} may reach {f.val:.3f}p, the header says < {lim}p")
    for f in (x, y):
        if f.val >= 2.0 or max(f.mx[:8]) > MASK:
            fail(f"{where}: {f.name} is not a multiplication output below 2 p")
    # a Jacobian base record (MulG1::load_base): zi = inv_fq(from_ext(z)), x = X zi^2, y = Y zi^3, then canonical(., 1)
    ext = Fe([MASK] * 8 + [(1 << 24) - 1], (1 << 256) / P, "ext")          # any 256-bit integer: unpack256
    cin = Fe([MASK] * 8 + [P >> 232], 1.0, "cin")
    z, X, Y = mul(ext, cin, "z"), mul(ext, cin, "X"), mul(ext, cin, "Y")
    zi = inv_fq(z, "zi")
    zi2 = sqr(zi, "zi2")
    bx, by = mul(X, zi2, "bx"), mul(Y, mul(zi2, zi, "zi3"), "by")
    for f in (z, bx, by):
        if f.val >= 2.0:
            fail(f"load_base: {f.name} may reach {f.val:.2f}p, canonical(., 1) takes values below 2 p")


NTTP_NEG = {"Y*one": 1.04, "-Y": 4.0}      # what the header of ntt_points.hip.h states for the negated T


def ntt_points(where="nttp_negate"):
    """ntt_points.hip.h.  A butterfly is T = mul_ladder(q, k) or pti_from_affi(q) on an unpacked canonical record -- the
    ladder of mul_points.hip.h, closed under the invariant --, then u + T and u - T = pti_madd(T or -T, u) with the
    canonical affine u: pti_madd on a point of the invariant and a canonical base, the case checked above with its
    doubling.  New is the negation of an XYZZ point whose Y may reach the invariant's 6 p, above the 3.9 p Fq29::neg
    takes: Y' = Y one (a product, below 1.04 p, exact 29-bit limbs), -Y' = norm(4 p - Y'); X, ZZ, ZZZ are T's own.  The
    result must be a point of the invariant again, because pti_madd takes it as its accumulator."""
    px, py, pzz, pzzz = point_invariant()
    one = Fe([MASK] * 8 + [P >> 232], 1.0, "one")
    y1 = mul(py, one, "Y*one")
    ny = neg(y1, "-Y")
    for f in (y1, ny):
        lim = NTTP_NEG[f.name]
        if f.val >= lim + MUL_NORM_SLACK:
            fail(f"{where}: {f.name} may reach {f.val:.3f}p, the header says < {lim}p")
    check_point(px, ny, pzz, pzzz, where)
    return {"Y*one": y1, "-Y": ny}


def contracts():
    """The operand contracts the headers state, whatever the caller: bn254_fq29.hip.h (mul / sqr: limbs <= 2^30 + 2^8,
    value <= 40 p; masked and wide digits) and bn254_fq2_29.hip.h (every operand of G2's mul / mul2 / sqr normalised:
    limbs 0..7 <= 2^29 + 8, limb 8 < 2^28, masked digits).  Returns the result bounds in multiples of p."""
    lazy = Fe([(1 << 30) + (1 << 8)] * 8 + [top_from_value(40.0)], 40.0, "lazy")
    g2 = Fe([MASK + 8] * 8 + [(1 << 28) - 1], 64.0, "normalised")
    out = {}
    for wide in (False, True):
        tag = " (wide)" if wide else ""
        out["mul" + tag] = mul(lazy, lazy, "lazy*lazy" + tag, wide)
        out["sqr" + tag] = sqr(lazy, "lazy^2" + tag, wide)
    out["mul2 (Fq2)"] = mul2(g2, g2, g2, g2, "Fq2 double product")
    # the folded forms at the same operand limit, the subtrahend anywhere under sub<K>'s contract (the tail is K - 0)
    for sel in KNAMES:
        x = Fe(KL[sel], KMULT[sel], "x")
        out[f"mul_sub<{sel}>"] = mul_sub(sel, lazy, lazy, x, f"lazy*lazy-x ({sel})")
        out[f"sqr_sub<{sel}>"] = sqr_sub(sel, lazy, x, f"lazy^2-x ({sel})")
    return out


def main(verbose=False):
    figures = {"operand contracts": contracts()}
    for bases in (PACKED, IN_PLACE):
        figures["pti_madd" + bases.tag] = pti_madd(bases)
        figures["pti_mmadd" + bases.tag] = pti_mmadd(bases)
    figures["pti_add_nz"] = pti_add_nz(INV_E)
    figures["pti_add_nz (E')"] = pti_add_nz(INV_ISO)
    mul_points()
    figures["nttp_negate"] = ntt_points()
    for site in sorted(derived_filters):
        print(f"zero filter {site}: needs {derived_filters[site]}, the header has {FILTERS.get(site)}")
    print(f"folded subtractions (mul_sub_np / sqr_sub_np): {len(folds)} uses, every one with wide digits, columns < 2^64 "
          f"with the tail, top limb inside 32 bits")
    if verbose:
        for where, fs in figures.items():
            print(where + ": " + ", ".join(f"{k} < {v.val:.2f} p" for k, v in fs.items()))
    if problems:
        print("LIMB BOUNDS VIOLATED:")
        for p in sorted(set(problems)):
            print("  -", p)
        return 1
    print("fq29 bounds: every column sum < 2^64, every lifted subtraction non-negative, every returned point within "
          "the invariant (pti_madd, pti_mmadd, pti_add_nz, pti_double); the shared inversion of mul_points.hip.h hands "
          "coordinates below 2 p to the packers")
    return 0


if __name__ == "__main__":
    sys.exit(main(verbose="-v" in sys.argv[1:]))
