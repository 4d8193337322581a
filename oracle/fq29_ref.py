"""Big-integer model of the 29-bit-limb internal representation of the hot kernels (csrc/bn254_fq29.hip.h: 9 limbs of
29 bits, lazily reduced, Montgomery radix rho = 2^261; csrc/bn254_ec29.hip.h: XYZZ points), with the postconditions
the headers state and corpus generators that put operands at the edges of the bounds contract.

p, the lifted constants K (`kc`) and the point invariant are not restated here: they come from the header through
tools/fq29_bounds.py (the interval proof of the same contract), so the proof and the tests share one set of numbers.
Records are the raw-limb layout of msm_amd_test_op_raw: 36 u32 per operand (a0 = words 0..8, a1 = 9..17; a point
X, Y, ZZ, ZZZ), 40 per result."""
import importlib.util
import os
import random
from fractions import Fraction

from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bounds():
    spec = importlib.util.spec_from_file_location("fq29_bounds", os.path.join(ROOT, "tools", "fq29_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FB = _load_bounds()
P = FB.P
assert P == o.P
PL, KL, KMULT, KNAMES = FB.PL, FB.KL, FB.KMULT, FB.KNAMES
INV = {"X": FB.INV_X, "Y": FB.INV_Y, "ZZ": FB.INV_ZZ, "ZZZ": FB.INV_ZZZ}
MASK, RHO = FB.MASK, FB.RHO
RHO_INV = pow(RHO, -1, P)
NEG_PINV_RHO = -pow(P, -1, RHO) % RHO
PINV29 = pow(P, -1, 1 << 29)
DOUT = (1 << 256) % P                      # to_ext's factor (the header's dout_c)

# the bounds contract of bn254_fq29.hip.h (header lines "Bounds contract") and bn254_ec29.hip.h
MUL_LIMB_MAX = (1 << 30) + (1 << 8)        # mul / sqr operand limbs
MUL_VALUE_MAX = 40 * P                     # mul / sqr operand value
NORM_LIMB_MAX = MASK + 8                   # limbs 0..7 after norm (< 2^29 + 8)
NEG_LIMB_MAX = (1 << 30) - 2               # neg / neg_wide operand limbs
U32 = (1 << 32) - 1

RAW_IN, RAW_OUT = 36, 40
(FE_MUL, FE_SQR, FE_MUL2, FE_SUB_K4E30, FE_SUB_K8E30, FE_SUB_K8E31, FE_SUB_K16E30, FE_SUB_K16E31, FE_NORM, FE_NEG,
 FE_NEG_WIDE, FE_CANONICAL, FE_TO_EXT, FE_PACK_UNPACK, FE_ZERO, PT_MADD, PT_MMADD, PT_ADD_NZ, PT_ADD,
 PT_DOUBLE) = range(20)
SUB_OPS = dict(zip((FE_SUB_K4E30, FE_SUB_K8E30, FE_SUB_K8E31, FE_SUB_K16E30, FE_SUB_K16E31), KNAMES))
OP_NAMES = {FE_MUL: "FE_MUL", FE_SQR: "FE_SQR", FE_MUL2: "FE_MUL2", FE_NORM: "FE_NORM", FE_NEG: "FE_NEG",
            FE_NEG_WIDE: "FE_NEG_WIDE", FE_CANONICAL: "FE_CANONICAL", FE_TO_EXT: "FE_TO_EXT",
            FE_PACK_UNPACK: "FE_PACK_UNPACK", FE_ZERO: "FE_ZERO", PT_MADD: "PT_MADD", PT_MMADD: "PT_MMADD",
            PT_ADD_NZ: "PT_ADD_NZ", PT_ADD: "PT_ADD", PT_DOUBLE: "PT_DOUBLE"}
OP_NAMES.update({op: "FE_SUB_" + k for op, k in SUB_OPS.items()})


# ---- values and limbs -------------------------------------------------------------------------------------------
def value(limbs):
    return sum(l << (29 * i) for i, l in enumerate(limbs))


def canon(v):
    """limbs 0..7 < 2^29 exactly, limb 8 the rest (the form a multiplication returns)"""
    assert 0 <= v < 1 << 264
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def words(v, n=8):
    return [(v >> (32 * i)) & U32 for i in range(n)]


def to_mont(x):
    return x * RHO % P


def from_mont(v):
    return v * RHO_INV % P


def mont(s):
    """Montgomery reduction of a product sum s with radix rho, digit by digit as reduce_columns does: the digits m_k
    depend only on s mod rho, so the result is exactly (s + m p) / rho with m = -s p^-1 mod rho."""
    return (s + (s * NEG_PINV_RHO % RHO) * P) // RHO


def top_for(low8, vmax):
    """largest top limb with value(low8 + [top]) <= vmax"""
    return (vmax - value(list(low8) + [0])) >> 232


def lift(v, bound):
    """v + k p with the largest k such that the result stays below bound * p (bound: a float of the invariant)"""
    lim = Fraction(str(bound)) * P
    k = int((lim - v - 1) // P)
    return v + max(k, 0) * P


def spread(v, rng, cmax, forced=None):
    """A lazy limb form of the value v: limb i = canon_i + c_i 2^29 - c_(i-1) with carries c_i in [0, cmax] (forced
    to 1 where a limb would go negative); limbs 0..7 < (cmax + 1) 2^29.  cmax = 1 keeps limbs below 2^30 (a valid
    mul operand), cmax = 7 below 2^32 (canonical's "arbitrary u32")."""
    c = canon(v)
    out, borrow = [], 0
    for i in range(8):
        cur = c[i] - borrow
        ci = forced if forced is not None else rng.randint(0, cmax)
        if cur < 0:
            ci = max(ci, 1)
        out.append(cur + (ci << 29))
        borrow = ci
    top = c[8] - borrow
    if top < 0:                 # no room above: give the last carry back
        out[7] -= borrow << 29
        if out[7] < 0:
            return canon(v)
        top += borrow
    out.append(top)
    assert value(out) == v
    return out


def borrowed(v):
    """v with every limb that can take a borrow from above inside the normalised bound (limbs 0..7 <= 2^29 + 7)
    taking it: a canonical limb l becomes 2^29 + l - (borrow it gave below).  Random values rarely allow one;
    small_limb_value builds values that allow all eight."""
    c = canon(v)
    out, borrow = [], 0
    for i in range(8):
        cur = c[i] - borrow
        ci = 1 if cur + (1 << 29) <= NORM_LIMB_MAX else 0
        if cur < 0:
            ci = 1
        out.append(cur + (ci << 29))
        borrow = ci
    out.append(c[8] - borrow)
    if out[8] < 0 or max(out[:8]) > NORM_LIMB_MAX:
        return canon(v)
    assert value(out) == v
    return out


def small_limb_value(lo_mult, hi_mult, rng):
    """A value in [lo_mult p, hi_mult p) whose limbs 0..7 are all <= 8 (limb 0 <= 7): its borrowed() form has every
    limb 0..7 at 2^29 + 7 or just below -- the largest limbs the normalised bound allows."""
    while True:
        low = [7] + [8] * 7 if rng.random() < 0.5 else [rng.randint(0, 7)] + [rng.randint(1, 8) for _ in range(7)]
        lo_t = -(-(lo_mult * P - value(low + [0])) >> 232)
        hi_t = (hi_mult * P - 1 - value(low + [0])) >> 232
        if lo_t <= hi_t:
            return value(low + [rng.randint(lo_t, hi_t)])


def sqrt_mod(a):
    """square root mod p (p = 3 mod 4) or None"""
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def rec(*fes):
    """one raw record: the field elements' limbs one after another, zero-padded to 36 words"""
    w = [l for fe in fes for l in fe]
    assert len(w) <= RAW_IN and all(0 <= x <= U32 for x in w), w
    return w + [0] * (RAW_IN - len(w))


# ---- the ops (exact limb models where the op is limb-wise, exact values where it is a reduction) --------------------
def sub_limbs(sel, a, b):
    """sub<K>(a, b) limb by limb, without wrapping: a limb outside [0, 2^32) is a broken precondition"""
    return [x + k - y for x, k, y in zip(a, KL[sel], b)]


def norm(a):
    r = [a[0] & MASK] + [(a[i] & MASK) + (a[i - 1] >> 29) for i in range(1, 8)]
    return r + [a[8] + (a[7] >> 29)]


def neg_wide(a):
    return sub_limbs("K4E30", [0] * 9, a)


def neg(a):
    return norm(neg_wide(a))


def canonical_value(v, rounds):
    return v - min(rounds, v // P) * P


def maybe_zero(l0, bound):
    return ((l0 & MASK) * PINV29) & MASK < bound


def filter_multiple(v):
    """j with v = j p, or None"""
    return v // P if v % P == 0 else None


# ---- points -------------------------------------------------------------------------------------------------------
def decode_point(words36):
    """XYZZ limbs -> bn254_ref affine point (None for ZZ limbs all zero); asserts ZZ^3 = ZZZ^2 and the curve."""
    X, Y, ZZ, ZZZ = (value(words36[9 * i:9 * i + 9]) for i in range(4))
    if not any(words36[18:27]):
        return None
    zz, zzz = from_mont(ZZ), from_mont(ZZZ)
    assert zz != 0 and pow(zz, 3, P) == pow(zzz, 2, P), "ZZ^3 != ZZZ^2"
    pt = (from_mont(X) * pow(zz, -1, P) % P, from_mont(Y) * pow(zzz, -1, P) % P)
    assert o.is_on_curve(pt), "result not on the curve"
    return pt


def point_post(words36):
    """the invariant of a stored / loop-carried point: X < 10 p, Y < 6 p, ZZ < 2.8 p, ZZZ < 2 p, limbs 0..7 <=
    2^29 + 7.  Returns a list of violations."""
    bad = []
    for i, name in enumerate(("X", "Y", "ZZ", "ZZZ")):
        f = words36[9 * i:9 * i + 9]
        if value(f) >= Fraction(str(INV[name])) * P:
            bad.append(f"{name} = {value(f) / P:.3f} p, the invariant says < {INV[name]} p")
        if max(f[:8]) > NORM_LIMB_MAX:
            bad.append(f"{name} has a limb {max(f[:8]):#x} above 2^29 + 7")
    return bad


def xyzz(pt, rng, lifts=(True, True, True, True), target=None, kx=None):
    """XYZZ limbs (4 x 9) of the affine point pt with a random Z, every coordinate lifted by the largest multiple
    of p the invariant allows (lifts[i] False: canonical; kx: X lifted by exactly kx p) and put in its borrowed form.
    target = "X" / "ZZ": Z is chosen so that that coordinate, lifted, has limbs 0..7 at the normalised maximum."""
    x, y = pt
    while True:
        if target is None:
            z = rng.randrange(1, P)
        else:
            k = {"X": (9 if lifts[0] else 0) if kx is None else kx, "ZZ": 2 if lifts[2] else 0}[target]
            hi = Fraction(str(INV[target])) * P
            hi_m = min(k + 1, int(-(-hi // P)))
            v = small_limb_value(k, hi_m, rng)
            if v >= hi:
                continue
            base = from_mont(v % P) * (pow(x, -1, P) if target == "X" else 1) % P
            z = sqrt_mod(base)
            if z is None or z == 0:
                continue
            if rng.random() < 0.5:
                z = P - z
        zz, zzz = z * z % P, z * z * z % P
        vals = [to_mont(x * zz % P), to_mont(y * zzz % P), to_mont(zz), to_mont(zzz)]
        out = []
        for i, (v, name) in enumerate(zip(vals, ("X", "Y", "ZZ", "ZZZ"))):
            if i == 0 and kx is not None:
                v = v + kx * P
            elif lifts[i]:
                v = lift(v, INV[name])
            out.append(borrowed(v))
        if target is not None:
            t = out[0] if target == "X" else out[2]
            assert min(t[:8]) >= 1 << 29, t
        return out


def affine_base(pt, wide_neg):
    """AffI register form of a base: canonical x, y (internal domain); wide_neg: the y register holds neg_wide of the
    stored -pt's y, as accumulate_kernel's signed_point leaves it (value 4 p - y', limbs up to 2^30.5)"""
    x, y = pt
    if wide_neg:
        return canon(to_mont(x)), neg_wide(canon(to_mont((-y) % P)))
    return canon(to_mont(x)), canon(to_mont(y))


def affine_of(xl, yl):
    return (from_mont(value(xl)), from_mont(value(yl)))


def classify(op, a, b):
    """(branch, j) the shipped formula takes for the raw records a, b: branch in generic / double / vanish /
    filter_pass (the one-limb filter passed a non-zero P), j the filter multiple value(P) / p when P = 0 mod p."""
    if op == PT_MADD:
        X1, Y1, ZZ1, ZZZ1 = (value(a[9 * i:9 * i + 9]) for i in range(4))
        qx, qy = value(b[0:9]), value(b[9:18])
        Pv = mont(qx * ZZ1) + KMULT["K16E30"] * P - X1
        Rv = mont(qy * ZZZ1) + KMULT["K8E30"] * P - Y1
        bound = 18
    elif op == PT_MMADD:
        Pv = value(b[0:9]) + KMULT["K16E30"] * P - value(a[0:9])
        Rv = value(b[9:18]) + KMULT["K8E30"] * P - value(a[9:18])
        bound = 18
    elif op == PT_ADD_NZ:
        X1, Y1, ZZ1, ZZZ1 = (value(a[9 * i:9 * i + 9]) for i in range(4))
        X2, Y2, ZZ2, ZZZ2 = (value(b[9 * i:9 * i + 9]) for i in range(4))
        Pv = mont(X2 * ZZ1) + KMULT["K4E30"] * P - mont(X1 * ZZ2)
        Rv = mont(Y2 * ZZZ1) + KMULT["K4E30"] * P - mont(Y1 * ZZZ2)
        bound = 6
    else:
        raise ValueError(op)
    assert Pv >= 0 and Rv >= 0
    if not maybe_zero(Pv & MASK, bound):
        return "generic", None
    j = filter_multiple(Pv)
    if j is None:
        return "filter_pass", None
    return ("double" if Rv % P == 0 else "vanish"), j


# the (op, branch, j) classes the point corpus claims to reach: every filter multiple the bounds allow
#   pti_madd: P = U2 + 16 p - X1 with U2 < 1.02 p, X1 = x + k p, k = 0..9 -> j = 16 + [U2 >= p] - k in 7..17
#   pti_mmadd: x1, x2 canonical -> j = 16
#   pti_add_nz: P = U2 + 4 p - U1, both < 1.3 p -> j in 3..5
CLAIMED = ({(PT_MADD, br, j) for br in ("double", "vanish") for j in range(7, 18)}
           | {(PT_MMADD, br, 16) for br in ("double", "vanish")}
           | {(PT_ADD_NZ, br, j) for br in ("double", "vanish") for j in (3, 4, 5)}
           | {(op, "generic", None) for op in (PT_MADD, PT_MMADD, PT_ADD_NZ)})


# ---- field-level corpus -------------------------------------------------------------------------------------------
def _rand_limbs(rng, limb_max, vmax, top_max=None):
    """random limbs 0..7 in [0, limb_max] (half of them near the maximum), top limb random under the value bound"""
    low = [limb_max - rng.randrange(1 << 8) if rng.random() < 0.5 else rng.randint(0, limb_max) for _ in range(8)]
    t = top_for(low, vmax)
    if top_max is not None:
        t = min(t, top_max)
    return low + [rng.randint(0, t) if t > 0 else 0]


def mul_operands(rng, n):
    """operands of mul / sqr at and inside the header's limit: limbs <= 2^30 + 2^8, value <= 40 p"""
    at_max = [MUL_LIMB_MAX] * 8
    at_max = at_max + [top_for(at_max, MUL_VALUE_MAX)]
    out = [at_max, [0] * 9, canon(P - 1), canon(1), spread(MUL_VALUE_MAX, rng, 1, forced=1),
           [MUL_LIMB_MAX] * 8 + [0], [0] * 8 + [top_for([0] * 8, MUL_VALUE_MAX)]]
    for _ in range(n):
        r = rng.random()
        if r < 0.4:
            out.append(_rand_limbs(rng, MUL_LIMB_MAX, MUL_VALUE_MAX))
        elif r < 0.7:
            out.append(spread(rng.randrange(MUL_VALUE_MAX + 1), rng, 1))
        else:
            out.append(canon(rng.randrange(P)))
    return out


def mul2_shapes(rng, n):
    """(a0, a1, b0, b1) of mul2 in the shape of pti_madd_tail / pti_mmadd_tail: R * T + Y1 * (-PPP) with R and Y1
    normalised (R < 12.1 p, Y1 < 6 p), T = Q + K16E30 - X3 un-normalised (Q a multiplication output < 1.2 p),
    -PPP = K4E30 - PPP (neg_wide, PPP >= 0).  The first record has every limb at its per-limb maximum."""
    kt, kn = KL["K16E30"], KL["K4E30"]
    q_top = (12 * P // 10) >> 232
    t_max = [MASK + k for k in kt[:8]] + [q_top + kt[8]]
    r_max = [NORM_LIMB_MAX] * 8
    r_max.append(top_for(r_max, 121 * P // 10))
    y_max = [NORM_LIMB_MAX] * 8
    y_max.append(top_for(y_max, 6 * P))
    out = [(r_max, t_max, y_max, list(kn))]
    for _ in range(n):
        q = canon(rng.randrange(12 * P // 10))
        x3 = _rand_limbs(rng, NORM_LIMB_MAX, 95 * P // 10)
        ppp = canon(rng.randrange(12 * P // 10))
        out.append((_rand_limbs(rng, NORM_LIMB_MAX, 121 * P // 10), sub_limbs("K16E30", q, x3),
                    _rand_limbs(rng, NORM_LIMB_MAX, 6 * P), neg_wide(ppp)))
    return out


def sub_operands(sel, rng, n):
    """(a, b) of sub<K>: subtrahend limbs <= the lifted K limbs, value <= k p; minuend limbs up to 2^32 - 1 - K_i"""
    K = KL[sel]
    amax = [U32 - k for k in K]
    out = [(amax, list(K)), ([0] * 9, list(K)), (amax, [0] * 9), ([0] * 9, [0] * 9)]
    for _ in range(n):
        b = [rng.randint(0, k) if rng.random() < 0.5 else k - rng.randrange(1 << 10) for k in K]
        while value(b) > KMULT[sel] * P:
            b[8] = rng.randint(0, b[8])
        a = [rng.randint(0, m) if rng.random() < 0.5 else m - rng.randrange(1 << 10) for m in amax]
        out.append((a, b))
    return out


def neg_operands(rng, n):
    """neg / neg_wide operands: limbs <= 2^30 - 2 (and <= the K4E30 limbs), value <= 4 p"""
    lim = [min(NEG_LIMB_MAX, k) for k in KL["K4E30"][:8]]
    at_max = lim + [top_for(lim, KMULT["K4E30"] * P)]
    # (a value near 4 p fits only with low limbs that took a borrow: K4E30's top limb is 4 p's minus 2)
    out = [at_max, [0] * 9, canon(3 * P), spread(4 * P - (1 << 233), rng, 1, forced=1), canon(P - 1)]
    for _ in range(n):
        low = [rng.randint(0, m) if rng.random() < 0.5 else m - rng.randrange(1 << 10) for m in lim]
        out.append(low + [rng.randint(0, max(top_for(low, 4 * P), 0))])
    return out


def norm_operands(rng, n):
    out = [[U32] * 8 + [U32 - 7], [U32] * 8 + [0], [1 << 29] * 9, [MASK] * 9]
    out += [[rng.randint(0, U32) for _ in range(8)] + [rng.randint(0, U32 - 7)] for _ in range(n)]
    return out


def canonical_operands(rng, n):
    """(limbs, rounds): arbitrary u32 limbs with value < (rounds + 1) p, incl. k p - 1, k p, k p + 1"""
    out = []
    for rounds in (0, 1, 2, 3, 8):
        for k in range(rounds + 1):
            for v in (k * P - 1, k * P, k * P + 1, (k + 1) * P - 1):
                if 0 <= v < (rounds + 1) * P:
                    out += [(canon(v), rounds), (spread(v, rng, 7), rounds), (spread(v, rng, 7, forced=7), rounds)]
    for _ in range(n):
        rounds = rng.choice((1, 2, 3, 8))
        v = rng.randrange((rounds + 1) * P)
        out.append((spread(v, rng, 7), rounds))
    return out


def pack_operands(rng, n):
    vals = [1 << k for k in range(256)] + [(1 << 256) - 1, 0, int("55" * 32, 16), int("AA" * 32, 16), P - 1]
    vals += [(1 << 256) - 1 - (1 << k) for k in range(0, 256, 5)]
    vals += [rng.getrandbits(256) for _ in range(n)]
    return [canon(v) for v in vals]


def zero_operands(rng, n):
    """(limbs, bound): j p for every j < bound in several limb forms (filter passes, exact test passes), the near
    misses j p + t 2^29 (filter passes, exact test fails), j = bound (filter fails), random non-zero values"""
    out = []
    for bound in (6, 18):
        for j in range(bound + 1):
            v = j * P
            out += [(canon(v), bound), (spread(v, rng, 1), bound), (spread(v, rng, 1, forced=1), bound),
                    (borrowed(v), bound)]
            for t in (1, 2, (1 << 20) + 3, rng.randrange(1, 1 << 200)):
                out.append((spread(v + (t << 29), rng, 1), bound))
            if j:
                out.append((spread(v - (1 << 29), rng, 1), bound))
        for _ in range(n):
            out.append((spread(rng.randrange(1, bound * P), rng, 1), bound))
    return out


def field_corpus(op, seed=0, n=200):
    """raw (a, b) records of one field op"""
    rng = random.Random(1000 * op + seed)
    if op in (FE_MUL, FE_SQR):
        ops = mul_operands(rng, n)
        other = list(reversed(ops))
        return [(rec(x), rec(y)) for x, y in zip(ops, other)] + [(rec(x), rec(x)) for x in ops[:8]]
    if op == FE_MUL2:
        return [(rec(r, t), rec(y, w)) for r, t, y, w in mul2_shapes(rng, n)]
    if op in SUB_OPS:
        return [(rec(a), rec(b)) for a, b in sub_operands(SUB_OPS[op], rng, n)]
    if op in (FE_NEG, FE_NEG_WIDE):
        return [(rec(a), rec([0] * 9)) for a in neg_operands(rng, n)]
    if op == FE_NORM:
        return [(rec(a), rec([0] * 9)) for a in norm_operands(rng, n)]
    if op == FE_CANONICAL:
        return [(rec(a), rec([r] + [0] * 8)) for a, r in canonical_operands(rng, n)]
    if op == FE_TO_EXT:
        return [(rec(a), rec([0] * 9)) for a in mul_operands(rng, n)]
    if op == FE_PACK_UNPACK:
        return [(rec(a), rec([0] * 9)) for a in pack_operands(rng, n)]
    if op == FE_ZERO:
        return [(rec(a), rec([bd] + [0] * 8)) for a, bd in zero_operands(rng, n // 10)]
    raise ValueError(op)


def field_pre(op, a, b):
    """the precondition a field record claims (violations as strings): what the corpus promises the code"""
    a0, a1, b0, b1 = a[0:9], a[9:18], b[0:9], b[9:18]
    bad = []

    def mul_ok(f, what):
        if max(f) > MUL_LIMB_MAX or value(f) > MUL_VALUE_MAX:
            bad.append(f"{what}: not a mul operand")
    if op in (FE_MUL, FE_SQR, FE_TO_EXT):
        mul_ok(a0, "a0")
        if op == FE_MUL:
            mul_ok(b0, "b0")
    elif op == FE_MUL2:
        for f, lim in ((a0, 121 * P // 10), (b0, 6 * P)):
            if max(f[:8]) > NORM_LIMB_MAX or value(f) >= lim:
                bad.append("normalised operand out of bounds")
        if any(x > MASK + k for x, k in zip(a1[:8], KL["K16E30"])) or value(a1) > 172 * P // 10 + (1 << 232):
            bad.append("T out of bounds")
        if any(x > k for x, k in zip(b1, KL["K4E30"])) or value(b1) > 4 * P:
            bad.append("-PPP out of bounds")
    elif op in SUB_OPS:
        sel = SUB_OPS[op]
        if any(y > k for y, k in zip(b0, KL[sel])) or value(b0) > KMULT[sel] * P:
            bad.append("subtrahend above the lift")
        if any(not 0 <= r <= U32 for r in sub_limbs(sel, a0, b0)):
            bad.append("a limb of the difference leaves 32 bits")
    elif op in (FE_NEG, FE_NEG_WIDE):
        if max(a0[:8]) > NEG_LIMB_MAX or any(x > k for x, k in zip(a0, KL["K4E30"])) or value(a0) > 4 * P:
            bad.append("neg operand out of bounds")
    elif op == FE_NORM:
        if a0[8] > U32 - 7:
            bad.append("top limb would wrap")
    elif op == FE_CANONICAL:
        if value(a0) >= (b0[0] + 1) * P:
            bad.append("value above (rounds + 1) p")
    elif op == FE_PACK_UNPACK:
        if max(a0[:8]) > MASK or value(a0) >= 1 << 256:
            bad.append("not canonical limbs")
    elif op == FE_ZERO:
        mul_ok(a0, "a0")
        if value(a0) >= max(b0[0], 1) * P and value(a0) % P == 0 and value(a0) // P > b0[0]:
            bad.append("multiple of p above the bound")
    return bad


def field_check(op, a, b, out):
    """violations of the model / the stated postconditions by one result record"""
    a0, a1, b0, b1 = a[0:9], a[9:18], b[0:9], b[9:18]
    r = out[0:9]
    bad = []
    if op in (FE_MUL, FE_SQR, FE_MUL2):
        s = {FE_MUL: value(a0) * value(b0), FE_SQR: value(a0) ** 2,
             FE_MUL2: value(a0) * value(a1) + value(b0) * value(b1)}[op]
        exp = canon(mont(s))
        if r != exp:
            bad.append(f"limbs {r} != model {exp} (a column overflowed or the reduction is wrong)")
        if (value(r) * RHO - s) % P or not 0 <= value(r) * RHO - s < P * RHO:
            bad.append("value is not (s + m p) / rho with m < rho")
        if max(r[:8]) > MASK:
            bad.append("limbs 0..7 not below 2^29")
    elif op in SUB_OPS:
        exp = sub_limbs(SUB_OPS[op], a0, b0)
        if r != exp:
            bad.append(f"limbs {r} != a + K - b limb by limb {exp} (a limb wrapped)")
        if value(r) != value(a0) + KMULT[SUB_OPS[op]] * P - value(b0):
            bad.append("value is not a + k p - b")
    elif op in (FE_NORM, FE_NEG, FE_NEG_WIDE):
        exp = {FE_NORM: norm, FE_NEG: neg, FE_NEG_WIDE: neg_wide}[op](a0)
        if r != exp:
            bad.append(f"limbs {r} != model {exp}")
        want = value(a0) if op == FE_NORM else 4 * P - value(a0)
        if value(r) != want:
            bad.append("value changed")
        if op != FE_NEG_WIDE and max(r[:8]) > NORM_LIMB_MAX:
            bad.append("limbs 0..7 above 2^29 + 7")
    elif op == FE_CANONICAL:
        v = canonical_value(value(a0), b0[0])
        if r != canon(v) or v >= P:
            bad.append(f"value {value(r)} != canonical {v}")
    elif op == FE_TO_EXT:
        m = mont(value(a0) * DOUT)
        m = m - P if m >= P else m
        want = value(a0) * (1 << 256) * RHO_INV % P
        if m != want or out[0:8] != words(want):
            bad.append(f"to_ext {out[0:8]} != {words(want)}")
    elif op == FE_PACK_UNPACK:
        if r != a0 or out[9:17] != words(value(a0)):
            bad.append("pack256 / unpack256 do not round-trip")
    elif op == FE_ZERO:
        want = [int(maybe_zero(a0[0], b0[0])), int(value(a0) % P == 0)]
        if out[0:2] != want:
            bad.append(f"(maybe_zero, is_zero_exact) = {out[0:2]} != {want}")
        if value(a0) % P == 0 and value(a0) // P < b0[0] and not out[0]:
            bad.append("the filter rejects a multiple of p below its bound")
    if any(out[{FE_TO_EXT: 8, FE_ZERO: 2, FE_PACK_UNPACK: 17}.get(op, 9):]):
        bad.append("words beyond the result are not zero")
    return bad


# ---- point-level corpus -------------------------------------------------------------------------------------------
def _rand_point(rng):
    return o.scalar_mul(rng.randrange(1, o.R_ORDER), o.GEN)


def point_corpus(op, seed=0, n=40):
    """[(a, b, expected affine, (branch, j))] for PT_MADD / PT_MMADD / PT_ADD_NZ / PT_ADD / PT_DOUBLE: points with
    random Z lifted to the invariant's edge (and borrowed limbs), bases canonical with y plain or as neg_wide; the
    partner random, equal (doubling) or opposite (vanish); for the claimed filter multiples j a search over Z and
    the X lift until the formula's P takes that multiple."""
    rng = random.Random(7000 + 100 * op + seed)
    out = []

    def add(a, b, exp):
        cls = classify(op, a, b) if op in (PT_MADD, PT_MMADD, PT_ADD_NZ) else (None, None)
        out.append((a, b, exp, cls))

    if op == PT_MADD:
        def one(p, q, rel, kx=None, target=None, wide=None):
            e = {"random": q, "equal": p, "opposite": o.aff_neg(p)}[rel]
            wide = rng.random() < 0.5 if wide is None else wide
            bx, by = affine_base(e, wide)
            a = rec(*xyzz(p, rng, kx=kx, target=target))
            add(a, rec(bx, by), o.aff_add(p, e))
            return out[-1][3]
        for i in range(n):
            p, q = _rand_point(rng), _rand_point(rng)
            one(p, q, "random", target=(None, "X", "ZZ")[i % 3])
            one(p, q, ("equal", "opposite")[i % 2], target=(None, "X", "ZZ")[i % 3])
        for rel, br in (("equal", "double"), ("opposite", "vanish")):
            for j in range(7, 18):
                for _ in range(4000):
                    p = _rand_point(rng)
                    kx = 16 - j if j < 17 else 0
                    if kx > 9:
                        break
                    got = one(p, p, rel, kx=kx)
                    if got == (br, j):
                        break
                    out.pop()
    elif op == PT_MMADD:
        for i in range(3 * n):
            p, q = _rand_point(rng), _rand_point(rng)
            rel = ("random", "equal", "opposite")[i % 3]
            e = {"random": q, "equal": p, "opposite": o.aff_neg(p)}[rel]
            px, py = affine_base(p, i % 2 == 0)
            py = norm(py)                               # the accumulator's y: normalised when it was stored
            bx, by = affine_base(e, (i // 2) % 2 == 0)
            add(rec(px, py), rec(bx, by), o.aff_add(p, e))
    elif op in (PT_ADD_NZ, PT_ADD):
        for i in range(3 * n):
            p, q = _rand_point(rng), _rand_point(rng)
            rel = ("random", "equal", "opposite")[i % 3]
            e = {"random": q, "equal": p, "opposite": o.aff_neg(p)}[rel]
            t1, t2 = (None, "X", "ZZ")[i % 3], (None, "ZZ", "X")[(i // 3) % 3]
            lifts = (True, True, True, True) if i % 4 else (False, False, False, False)
            add(rec(*xyzz(p, rng, lifts=lifts, target=t1)), rec(*xyzz(e, rng, target=t2)), o.aff_add(p, e))
        if op == PT_ADD_NZ:
            for rel, br in (("equal", "double"), ("opposite", "vanish")):
                for j in (3, 4, 5):
                    for _ in range(4000):
                        p = _rand_point(rng)
                        e = p if rel == "equal" else o.aff_neg(p)
                        add(rec(*xyzz(p, rng)), rec(*xyzz(e, rng)), o.aff_add(p, e))
                        if out[-1][3] == (br, j):
                            break
                        out.pop()
        else:
            ident = rec(canon(to_mont(1)), canon(to_mont(1)), [0] * 9, [0] * 9)
            p = _rand_point(rng)
            add(ident, rec(*xyzz(p, rng)), p)
            add(rec(*xyzz(p, rng)), ident, p)
            add(ident, ident, None)
    elif op == PT_DOUBLE:
        for i in range(2 * n):
            p = _rand_point(rng)
            add(rec(*xyzz(p, rng, target=(None, "X", "ZZ")[i % 3])), rec([0] * 9), o.aff_add(p, p))
    else:
        raise ValueError(op)
    return out


def point_check(op, a, b, out, exp, cls):
    """violations by one point result: the decoded sum, the invariant, the vanished flag"""
    bad = []
    try:
        got = decode_point(out[0:36])
    except AssertionError as e:
        return [f"result not a valid XYZZ point: {e}"]
    if got != exp:
        bad.append(f"sum {got} != oracle {exp}")
    bad += point_post(out[0:36])
    if op in (PT_MADD, PT_MMADD, PT_ADD_NZ):
        if out[36] != int(cls[0] == "vanish"):
            bad.append(f"vanished = {out[36]} for branch {cls}")
    elif out[36]:
        bad.append("word 36 set")
    if any(out[37:]):
        bad.append("words beyond the result are not zero")
    return bad


def point_pre(op, a, b):
    """the precondition a point record claims"""
    bad = []
    pts = [a[0:36]] if op in (PT_MADD, PT_DOUBLE) else ([a[0:36], b[0:36]] if op in (PT_ADD_NZ, PT_ADD) else [])
    for w in pts:
        if any(w[18:27]):
            bad += point_post(w)
    if op in (PT_MADD, PT_MMADD):
        bx, by = b[0:9], b[9:18]
        if value(bx) >= P or max(bx[:8]) > MASK:
            bad.append("base x not canonical")
        if not (value(by) < P and max(by[:8]) <= MASK) and any(y > k for y, k in zip(by, KL["K4E30"])):
            bad.append("base y neither canonical nor a neg_wide value")
    if op == PT_MMADD:
        if value(a[0:9]) >= P or max(a[0:8]) > MASK:
            bad.append("px not canonical")
        if value(a[9:18]) >= 4 * P or max(a[9:17]) > NORM_LIMB_MAX:
            bad.append("py not a normalised base y")
    return bad
