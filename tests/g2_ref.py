"""Big-integer model of BN254 G2 for the G2 tests: Fq2 = Fq[u] / (u^2 + 1), the twist y^2 = x^3 + 3 / (9 + u), affine
group law, scalar multiplication, the external byte layouts (halo2curves G2Affine 128 B, ark G2Affine 136 B, the
192-byte Jacobian result) and the raw-limb records of msm_amd_test_op_g2 (29-bit internal limbs, rho = 2^261).
No MSM code: this is what the library's G2 results are checked against."""
import random

from oracle import bn254_ref as o
from oracle import fq29_ref as f

P = o.P
R_ORDER = o.R_ORDER
MONT_R = o.MONT_R
RHO = 1 << 261
RHO_INV = pow(RHO, -1, P)


# ---- Fq2 (pairs of ints mod p) --------------------------------------------------------------------------------------
def add2(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub2(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul2(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def inv2(a):
    t = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * t % P, -a[1] * t % P)


def neg2(a):
    return ((-a[0]) % P, (-a[1]) % P)


ZERO2, ONE2 = (0, 0), (1, 0)
B_TWIST = mul2((3, 0), inv2((9, 1)))      # b' = 3 / (9 + u)

# EIP-197 generator of G2
GEN2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
         11559732032986387107991004021392285783925812861821192530917403151452391805634),
        (8495653923123431417604973247489272438418190587263600148770280649306958101930,
         4082367875863433681332203403145435568316851327593401208105741076214120093531))


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return mul2(y, y) == add2(mul2(mul2(x, x), x), B_TWIST)


# ---- affine group law (None = identity) -----------------------------------------------------------------------------
def neg(pt):
    return None if pt is None else (pt[0], neg2(pt[1]))


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        if p1[1] != p2[1] or p1[1] == ZERO2:
            return None
        lam = mul2(mul2((3, 0), mul2(p1[0], p1[0])), inv2(add2(p1[1], p1[1])))
    else:
        lam = mul2(sub2(p2[1], p1[1]), inv2(sub2(p2[0], p1[0])))
    x3 = sub2(sub2(mul2(lam, lam), p1[0]), p2[0])
    return (x3, sub2(mul2(lam, sub2(p1[0], x3)), p1[1]))


def _jdbl(p):
    x, y, z = p
    if z == ZERO2:
        return p
    a, b = mul2(x, x), mul2(y, y)
    c = mul2(b, b)
    d = mul2((2, 0), sub2(sub2(mul2(add2(x, b), add2(x, b)), a), c))
    e = mul2((3, 0), a)
    x3 = sub2(mul2(e, e), add2(d, d))
    y3 = sub2(mul2(e, sub2(d, x3)), mul2((8, 0), c))
    return (x3, y3, mul2((2, 0), mul2(y, z)))


def _to_affine_j(p):
    x, y, z = p
    if z == ZERO2:
        return None
    zi = inv2(z)
    zi2 = mul2(zi, zi)
    return (mul2(x, zi2), mul2(y, mul2(zi2, zi)))


def _jadd_aff(p, q):
    """Jacobian p + affine q (q not the identity)"""
    x1, y1, z1 = p
    if z1 == ZERO2:
        return (q[0], q[1], ONE2)
    z1z1 = mul2(z1, z1)
    u2, s2 = mul2(q[0], z1z1), mul2(q[1], mul2(z1, z1z1))
    h, r = sub2(u2, x1), sub2(s2, y1)
    if h == ZERO2:
        return _jdbl(p) if r == ZERO2 else (ONE2, ONE2, ZERO2)
    hh = mul2(h, h)
    hhh = mul2(h, hh)
    v = mul2(x1, hh)
    x3 = sub2(sub2(mul2(r, r), hhh), add2(v, v))
    y3 = sub2(mul2(r, sub2(v, x3)), mul2(y1, hhh))
    return (x3, y3, mul2(z1, h))


def scalar_mul(k, pt):
    """k pt for any integer k >= 0 (not reduced mod r: r G2 = O is a test of the model), Jacobian double-and-add"""
    if pt is None or k == 0:
        return None
    acc = (ONE2, ONE2, ZERO2)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd_aff(acc, pt)
    return _to_affine_j(acc)


def msm_naive(scalars, points):
    acc = None
    for k, pt in zip(scalars, points):
        acc = add(acc, scalar_mul(k, pt))
    return acc


# ---- external layouts -----------------------------------------------------------------------------------------------
def _le(x):
    return (x % (1 << 256)).to_bytes(32, "little")


def encode_h2c(pt) -> bytes:
    if pt is None:
        return bytes(128)
    (x0, x1), (y0, y1) = pt
    return b"".join(_le(o.fq_to_mont(v)) for v in (x0, x1, y0, y1))


def encode_ark(pt) -> bytes:
    if pt is None:
        return bytes(128) + b"\x01" + bytes(7)
    return encode_h2c(pt) + bytes(8)


def decode_h2c(buf: bytes):
    v = [o.fq_from_mont(int.from_bytes(buf[32 * i:32 * i + 32], "little")) for i in range(4)]
    if buf[:128] == bytes(128):
        return None
    return ((v[0], v[1]), (v[2], v[3]))


def decode_jacobian(buf: bytes):
    """192-byte Montgomery Jacobian -> affine ((x0, x1), (y0, y1)) or None."""
    assert len(buf) == 192
    v = [o.fq_from_mont(int.from_bytes(buf[32 * i:32 * i + 32], "little")) for i in range(6)]
    return _to_affine_j(((v[0], v[1]), (v[2], v[3]), (v[4], v[5])))


def identity_bytes() -> bytes:
    one = _le(o.fq_to_mont(1))
    return one + bytes(32) + one + bytes(32) + bytes(64)


def encode_scalar(k: int, layout: int) -> bytes:
    """MSM_AMD_SCALAR_MONT_LE (0), CANON_LE (1), CANON_BE32 (2)."""
    if layout == 0:
        return _le(o.fr_to_mont(k % R_ORDER))
    if layout == 1:
        return _le(k)
    be = k.to_bytes(32, "big")
    return b"".join(be[4 * i:4 * i + 4][::-1] for i in range(8))   # 8 x u32 MS limb first, each a host-order word


# ---- raw-limb records (29-bit limbs, internal Montgomery domain rho = 2^261) --------------------------------------------
def limbs_of(v, bound=None, rng=None):
    """Limbs of the integer v (0 <= v), plain 29-bit slicing, or, with rng, one of the limb vectors of the same value
    that borrows from the upper limbs (limbs 0..7 up to 2^29 + 7: the normalised maximum)."""
    l = [(v >> (29 * i)) & f.MASK for i in range(8)] + [v >> 232]
    if rng is not None:
        for i in range(8):
            if l[i + 1] > 0 and rng.random() < 0.5 and l[i] + (1 << 29) <= f.NORM_LIMB_MAX:
                l[i] += 1 << 29
                l[i + 1] -= 1
    return l


def value(limbs):
    return sum(x << (29 * i) for i, x in enumerate(limbs))


def fe_rec(x_int, mult, rng):
    """a limb vector of the internal form of x (x rho mod p) plus j p for a random j < mult (the bounds contract's edge
    is reached when j = mult - 1), limbs normalised."""
    base = x_int * RHO % P
    j = mult - 1 if rng.random() < 0.5 else rng.randrange(mult)
    v = base + j * P
    return limbs_of(v, rng=rng)


def fq2_rec(a, mult, rng):
    m0, m1 = mult if isinstance(mult, tuple) else (mult, mult)
    return fe_rec(a[0], m0, rng) + fe_rec(a[1], m1, rng)


def fq2_of(words):
    """actual Fq2 value of an 18-word internal record"""
    return (value(words[:9]) * RHO_INV % P, value(words[9:18]) * RHO_INV % P)


def rand_fq2(rng):
    return (rng.randrange(P), rng.randrange(P))


def rand_point(rng):
    return scalar_mul(rng.randrange(1, R_ORDER), GEN2)


# Bounds of the contract (bn254_ec2_29.hip.h): X < 1.21 p, Y < 13.4 p, ZZ < 3.2 p, ZZZ < 2.04 p; affine bases
# canonical with y possibly negated (< 4 p)
PT_MULT = {"y": 13, "zz": 3, "zzz": 2}   # j < mult extra multiples of p: Y < 13 p, ZZ < 3 p, ZZZ < 2 p


def xyzz_rec(pt, rng, z=None):
    """XYZZ record of the affine point pt with a random Z: X = x Z^2, Y = y Z^3, each coordinate at a random multiple of
    p inside the invariant"""
    z = z or rand_fq2(rng)
    zz = mul2(z, z)
    zzz = mul2(zz, z)
    X, Y = mul2(pt[0], zz), mul2(pt[1], zzz)
    # X < 1.21 p leaves no room for a whole extra p; the others get random multiples
    return (limbs_of(X[0] * RHO % P) + limbs_of(X[1] * RHO % P) + fq2_rec(Y, PT_MULT["y"], rng) +
            fq2_rec(zz, PT_MULT["zz"], rng) + fq2_rec(zzz, PT_MULT["zzz"], rng))


def aff_rec(pt, rng, negated=False):
    """affine base record: canonical x, y; negated: 4 p - y limb form (the accumulate kernel's signed base)"""
    x, y = pt
    xs = limbs_of(x[0] * RHO % P) + limbs_of(x[1] * RHO % P)
    if negated:
        ys = limbs_of(4 * P - y[0] * RHO % P) + limbs_of(4 * P - y[1] * RHO % P)
        return xs + ys, (x, neg2(y))
    return xs + limbs_of(y[0] * RHO % P) + limbs_of(y[1] * RHO % P), pt


def decode_xyzz(words):
    """affine point of a 72-word XYZZ record: x = X / ZZ, y = Y / ZZZ (the Montgomery factors cancel)"""
    X = (value(words[0:9]) % P, value(words[9:18]) % P)
    Y = (value(words[18:27]) % P, value(words[27:36]) % P)
    ZZ = (value(words[36:45]) % P, value(words[45:54]) % P)
    ZZZ = (value(words[54:63]) % P, value(words[63:72]) % P)
    if ZZ == ZERO2:
        return None
    return (mul2(X, inv2(ZZ)), mul2(Y, inv2(ZZZ)))


def pad(words, n=72):
    return list(words) + [0] * (n - len(words))


def component_multiples(words, count):
    """value of each 9-limb component / p, for the bound checks"""
    return [value(words[9 * i:9 * i + 9]) / P for i in range(count)]


def normalised(words, count):
    return all(words[9 * i + k] <= f.NORM_LIMB_MAX for i in range(count) for k in range(8))


def rng_for(seed):
    return random.Random(seed)
