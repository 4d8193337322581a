"""Big-integer model of the BN254 pairing for the pairing tests, on g2_ref.py's Fq2.

Fq12 here is Fq2[w] / (w^6 - xi), xi = 9 + u: six Fq2 coefficients of w^0 .. w^5 and a plain polynomial product, so the
model shares nothing with the towers of the library (Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v), v = w^2).
The tower coefficient c_h.c_k (h < 2, k < 3) is the coefficient of w^(2k + h); the 384-byte GT record lists c0.c0,
c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each an Fq2 (c0 then c1) of 32-byte little-endian fields.

The Miller loop is the textbook one: affine points on the twist, plain binary double-and-add over 6x + 2, a line
through two points by its slope, evaluated at P through the untwist (x, y) -> (x w^2, y w^3), then the two Frobenius
steps of the optimal ate pairing.  The final exponentiation is the plain power by (p^12 - 1) / r.  The library uses
projective, division-free steps over signed digits and an x-power chain: only the GT element can be compared, a Miller
value is compared after the model's final exponentiation.

Also here: the limb-level mirror of msm_amd_test_fq12_op (records of 108 raw 29-bit limbs in the tower order) with
operands at chosen multiples of p (fe_rec / fq2_rec of g2_ref.py)."""
import json
import os
import random

from oracle import bn254_ref as o
import g2_ref as g2

P = o.P
R_ORDER = o.R_ORDER
X_BN = 4965661367192848881
assert P == 36 * X_BN**4 + 36 * X_BN**3 + 24 * X_BN**2 + 6 * X_BN + 1
assert R_ORDER == 36 * X_BN**4 + 36 * X_BN**3 + 18 * X_BN**2 + 6 * X_BN + 1
ATE = 6 * X_BN + 2
FINAL_EXPONENT = (P**12 - 1) // R_ORDER
assert (P**12 - 1) % R_ORDER == 0
XI = (9, 1)

add2, sub2, mul2, inv2, neg2 = g2.add2, g2.sub2, g2.mul2, g2.inv2, g2.neg2
ZERO2, ONE2 = g2.ZERO2, g2.ONE2

GT_MONT_LE, GT_CANON_LE = 0, 1
PAIRING_MILLER_ONLY = 1
GT_BYTES = 384
# msm_amd_test_fq12_op
(FQ12_OP_FQ6_MUL, FQ12_OP_MUL, FQ12_OP_SQR, FQ12_OP_CYCLO_SQR, FQ12_OP_LINE_MUL, FQ12_OP_FROB1, FQ12_OP_FROB2,
 FQ12_OP_FROB3, FQ12_OP_CONJ, FQ12_OP_INV, FQ12_OP_POW_X, FQ12_OP_DOUBLE_STEP, FQ12_OP_ADD_STEP,
 FQ12_OP_FINAL_EXP) = range(14)
FQ12_WORDS = 108


def conj2(a):
    return (a[0], (-a[1]) % P)


def pow2(a, e):
    r = ONE2
    for bit in bin(e)[2:]:
        r = mul2(r, r)
        if bit == "1":
            r = mul2(r, a)
    return r


# ---- Fq12 = Fq2[w] / (w^6 - xi): tuples of six Fq2 -------------------------------------------------------------------
ONE12 = (ONE2,) + (ZERO2,) * 5
ZERO12 = (ZERO2,) * 6


def mul12(a, b):
    t = [ZERO2] * 11
    for i in range(6):
        if a[i] == ZERO2:
            continue
        for j in range(6):
            t[i + j] = add2(t[i + j], mul2(a[i], b[j]))
    return tuple(add2(t[k], mul2(XI, t[k + 6])) if k < 5 else t[k] for k in range(6))


def sqr12(a):
    return mul12(a, a)


def pow12(a, e):
    r = ONE12
    for bit in bin(e)[2:]:
        r = sqr12(r)
        if bit == "1":
            r = mul12(r, a)
    return r


def conj12(a):
    """a^(p^6): w -> -w"""
    return tuple(a[i] if i % 2 == 0 else neg2(a[i]) for i in range(6))


# gamma[k][i] = xi^(i (p^k - 1) / 6): Frobenius^k sends a_i w^i to conj^k(a_i) gamma[k][i] w^i
GAMMA = {k: [pow2(XI, i * (P**k - 1) // 6) for i in range(6)] for k in (1, 2, 3)}


def frob12(a, k):
    return tuple(mul2(conj2(a[i]) if k % 2 else a[i], GAMMA[k][i]) for i in range(6))


def inv12(a):
    """a^-1 by a^(p^12 - 2) would cost 3000 squarings; use the norm chain instead: b = product of the five conjugates over
    Fq2 (a^(p^2), a^(p^4), ...), a b in Fq2."""
    c = ONE12
    t = a
    for _ in range(5):
        t = frob12(t, 2)
        c = mul12(c, t)
    n = mul12(a, c)
    assert n[1:] == (ZERO2,) * 5
    ni = inv2(n[0])
    return tuple(mul2(x, ni) for x in c)


def final_exponentiation(f):
    return pow12(f, FINAL_EXPONENT)


def gt_pow(g, e):
    return pow12(g, e % R_ORDER)


# ---- the optimal ate Miller function --------------------------------------------------------------------------------
def _line(t, q, p1):
    """the line through the twist points t, q (tangent when equal), evaluated at the G1 point p1 through the untwist;
    None for a vertical line (a factor of a subfield: the final exponentiation kills it)"""
    (x1, y1), (x2, y2) = t, q
    if x1 == x2:
        if y1 != y2 or y1 == ZERO2:
            return None
        lam = mul2(mul2((3, 0), mul2(x1, x1)), inv2(add2(y1, y1)))
    else:
        lam = mul2(sub2(y2, y1), inv2(sub2(x2, x1)))
    xp, yp = p1
    # y_P - y_T w^3 - lam w (x_P - x_T w^2)
    return ((yp, 0), neg2(mul2(lam, (xp, 0))), ZERO2, sub2(mul2(lam, x1), y1), ZERO2, ZERO2)


def frob_twist(q, k=1):
    """the p^k-power Frobenius on the twist: untwist, Frobenius, twist"""
    x, y = q
    if k % 2:
        x, y = conj2(x), conj2(y)
    return (mul2(x, GAMMA[k][2]), mul2(y, GAMMA[k][3]))


def miller_loop(p1, q):
    """f_{6x+2,Q}(P) l_{T,pi(Q)}(P) l_{T+pi(Q),-pi^2(Q)}(P); p1 affine G1 (x, y) or None, q affine G2 or None"""
    if p1 is None or q is None:
        return ONE12
    f, t = ONE12, q
    for bit in bin(ATE)[3:]:
        f = sqr12(f)
        l = _line(t, t, p1)
        f = mul12(l, f) if l else f
        t = g2.add(t, t)
        if bit == "1":
            l = _line(t, q, p1)
            f = mul12(l, f) if l else f
            t = g2.add(t, q)
    q1 = frob_twist(q, 1)
    q2 = g2.neg(frob_twist(q, 2))
    l = _line(t, q1, p1)
    f = mul12(l, f) if l else f
    t = g2.add(t, q1)
    l = _line(t, q2, p1)
    f = mul12(l, f) if l else f
    return f


def pairing(p1, q):
    return final_exponentiation(miller_loop(p1, q))


def pairing_product(pairs):
    f = ONE12
    for p1, q in pairs:
        f = mul12(f, miller_loop(p1, q))
    return final_exponentiation(f)


# ---- the record codecs -------------------------------------------------------------------------------------------------
def _tower_order(a):
    """the six Fq2 of the record: c_h.c_k = coefficient of w^(2k + h)"""
    return [a[2 * k + h] for h in range(2) for k in range(3)]


def _from_tower(cs):
    a = [None] * 6
    for r, c in enumerate(cs):
        h, k = divmod(r, 3)
        a[2 * k + h] = c
    return tuple(a)


def encode_gt(a, layout=GT_MONT_LE) -> bytes:
    out = b""
    for c in _tower_order(a):
        for v in c:
            out += ((o.fq_to_mont(v) if layout == GT_MONT_LE else v) % P).to_bytes(32, "little")
    return out


def decode_gt(buf: bytes, layout=GT_MONT_LE):
    assert len(buf) == GT_BYTES
    v = [int.from_bytes(buf[32 * i:32 * i + 32], "little") for i in range(12)]
    assert all(x < P for x in v), "not canonical"
    if layout == GT_MONT_LE:
        v = [o.fq_from_mont(x) for x in v]
    return _from_tower([(v[2 * i], v[2 * i + 1]) for i in range(6)])


# ---- golden file: e(G1, G2) and two more pairs ----------------------------------------------------------------------------
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairing_known.json")
GOLDEN_SCALARS = ((1, 1), (2, 3), (0x1234567, 0x89ABCDEF0123))


def g1_mul(k):
    return o.scalar_mul(k, o.GEN)


def g2_mul(k):
    return g2.scalar_mul(k % R_ORDER, g2.GEN2)


def golden_entries():
    out = []
    for a, b in GOLDEN_SCALARS:
        p1, q = g1_mul(a), g2_mul(b)
        e = pairing(p1, q)
        out.append({"a": hex(a), "b": hex(b), "g1_h2c_affine": o.encode_affine_h2c(p1).hex(),
                    "g2_h2c_affine": g2.encode_h2c(q).hex(), "gt_mont_le": encode_gt(e, GT_MONT_LE).hex(),
                    "gt_canon_le": encode_gt(e, GT_CANON_LE).hex()})
    return out


_G = None


def gt_generator():
    """e(G1, G2), read from the golden file (tests/test_pairing_host.py checks the file against the model)"""
    global _G
    if _G is None:
        d = json.load(open(GOLDEN_PATH))
        _G = decode_gt(bytes.fromhex(d["pairs"][0]["gt_canon_le"]), GT_CANON_LE)
    return _G


def expected_by_dlog(scalar_pairs):
    """e-product of the pairs (a_i G1, b_i G2): g^(sum a_i b_i mod r), one GT power instead of n Miller loops"""
    return gt_pow(gt_generator(), sum(a * b for a, b in scalar_pairs) % R_ORDER)


# ---- limb-level mirror of msm_amd_test_fq12_op ---------------------------------------------------------------------------
RHO = g2.RHO
B3 = mul2((9, 0), inv2(XI))      # 3 b' = 9 / xi


def fq12_rec(a, mult, rng):
    """108 raw limbs of a (tower order), every component at a multiple of p below mult"""
    words = []
    for c in _tower_order(a):
        words += g2.fq2_rec(c, mult, rng)
    return words


def fq12_of(words):
    return _from_tower([g2.fq2_of(words[18 * i:18 * i + 18]) for i in range(6)])


def rand_fq12(rng):
    return tuple(g2.rand_fq2(rng) for _ in range(6))


def rand_cyclotomic(rng):
    """an element of the cyclotomic subgroup: f^((p^6 - 1)(p^2 + 1))"""
    f = rand_fq12(rng)
    t = mul12(conj12(f), inv12(f))
    return mul12(frob12(t, 2), t)


def line12(l0, l1, l3):
    return (l0, l1, ZERO2, l3, ZERO2, ZERO2)


def double_step(t, p1):
    """the projective doubling step of the library (homogeneous X, Y, Z on the twist) and its line (l0, l1, l3) at P"""
    X, Y, Z = t
    xp, yp = p1
    b, c = mul2(Y, Y), mul2(Z, Z)
    e = mul2(B3, c)
    f = mul2((3, 0), e)
    h = mul2((2, 0), mul2(Y, Z))
    i = sub2(e, b)
    j = mul2(X, X)
    X3 = mul2(mul2((2, 0), mul2(X, Y)), sub2(b, f))
    Y3 = sub2(mul2(add2(b, f), add2(b, f)), mul2((12, 0), mul2(e, e)))
    Z3 = mul2((4, 0), mul2(b, h))
    return (X3, Y3, Z3), (mul2(h, ((-yp) % P, 0)), mul2(mul2((3, 0), j), (xp, 0)), i)


def add_step(t, q, p1):
    """T + Q, Q affine, and the line through them at P"""
    X, Y, Z = t
    qx, qy = q
    xp, yp = p1
    theta = sub2(Y, mul2(qy, Z))
    lam = sub2(X, mul2(qx, Z))
    c, d = mul2(theta, theta), mul2(lam, lam)
    e = mul2(lam, d)
    f = mul2(Z, c)
    g = mul2(X, d)
    h = sub2(add2(e, f), add2(g, g))
    X3 = mul2(lam, h)
    Y3 = sub2(mul2(theta, sub2(g, h)), mul2(e, Y))
    Z3 = mul2(Z, e)
    j = sub2(mul2(theta, qx), mul2(lam, qy))
    return (X3, Y3, Z3), (mul2(lam, (yp, 0)), mul2(theta, ((-xp) % P, 0)), j)


def proj_to_affine(t):
    X, Y, Z = t
    if Z == ZERO2:
        return None
    zi = inv2(Z)
    return (mul2(X, zi), mul2(Y, zi))


def rng_for(seed):
    return random.Random(seed)


if __name__ == "__main__":   # PYTHONPATH=.:tests python tests/pairing_ref.py rewrites the golden file from the model
    doc = {"what": "BN254 optimal ate pairings e(a G1, b G2) computed by the big-integer model of tests/pairing_ref.py: "
                   "f^((p^12 - 1) / r) exactly, records of 12 x 32 bytes in the order c0.c0.c0 .. c1.c2.c1, little-endian",
           "g1_generator": "(1, 2)", "g2_generator": "EIP-197", "pairs": golden_entries()}
    with open(GOLDEN_PATH, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
