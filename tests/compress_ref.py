"""Big-integer model of the compressed point formats (msm_amd_decompress_points*, msm_amd_compress_points*): encode and
decode of both formats for both groups, the reason code of a record, the expected output records of every host layout,
and the planted cases -- each found by the model itself (a search upwards from a seed), none skipped.  check_ref, g2_ref
and oracle.bn254_ref are used unchanged."""
import random

import check_ref as c
import g2_ref as g
from oracle import bn254_ref as o

P = o.P
ARK, PARITY = 0, 1                                         # MSM_AMD_COMPRESSED_*
VALID, NOT_REDUCED, NOT_ON_CURVE, NOT_IN_SUBGROUP, BAD_ENCODING = range(5)
HALF = (P - 1) // 2
TOP = 1 << 254                                             # the two flag bits sit at 2^254 (0x40) and 2^255 (0x80)
SIZE = {1: 32, 2: 64}
OUT_BYTES = {(1, c.H2C): 64, (1, c.ARK_AFFINE): 72, (2, c.G2_H2C): 128, (2, c.G2_ARK): 136}
B1 = 3


# ---- the sign rules ---------------------------------------------------------------------------------------------------
def sign(group, fmt, y):
    """the flag bit of y under the format's rule"""
    if group == 1:
        return int(y > HALF) if fmt == ARK else y & 1
    y0, y1 = y
    if fmt == ARK:                                         # y > -y, c1 compared first
        return int(y1 > HALF) if y1 else int(y0 > HALF)
    return (y0 if y0 else y1) & 1


def neg_y(group, y):
    return -y % P if group == 1 else g.neg2(y)


def flag_bits(fmt, ident, s):
    if ident:
        return 0x40 if fmt == ARK else 0x80
    return (0x80 if fmt == ARK else 0x40) if s else 0


def rhs(group, x):
    if group == 1:
        return (x * x * x + B1) % P
    return g.add2(g.mul2(g.mul2(x, x), x), g.B_TWIST)


def root(group, a):
    return c.sqrt_fq(a) if group == 1 else c.sqrt_fq2(a)


# ---- records ------------------------------------------------------------------------------------------------------------
def raw_record(group, xs, flags):
    """xs: the stored integer(s) below 2^254 (G2: c0 may be anything below 2^256), flags: the top two bits as 0x80 | 0x40"""
    if group == 1:
        assert xs < TOP
        return (xs | (flags >> 6) << 254).to_bytes(32, "little")
    x0, x1 = xs
    assert x1 < TOP and x0 < (1 << 256)
    return x0.to_bytes(32, "little") + (x1 | (flags >> 6) << 254).to_bytes(32, "little")


def encode(group, fmt, pt):
    """affine point (None = identity) -> compressed record"""
    if pt is None:
        return raw_record(group, 0 if group == 1 else (0, 0), flag_bits(fmt, True, 0))
    return raw_record(group, pt[0], flag_bits(fmt, False, sign(group, fmt, pt[1])))


def split(group, fmt, rec):
    """record -> (x integers after masking, identity flag, sign flag)"""
    last = rec[-1]
    hi, lo = last >> 7, (last >> 6) & 1
    ident, s = (lo, hi) if fmt == ARK else (hi, lo)
    body = rec[:-1] + bytes([last & 0x3F])
    xs = [int.from_bytes(body[32 * i:32 * i + 32], "little") for i in range(group)]
    return xs, ident, s


def decode(group, fmt, rec):
    """-> (reason, point or None); the first rule that fails"""
    xs, ident, s = split(group, fmt, rec)
    if (ident and s) or (ident and any(xs)):
        return BAD_ENCODING, None
    if ident:
        return VALID, None
    if any(x >= P for x in xs):
        return NOT_REDUCED, None
    x = xs[0] if group == 1 else (xs[0], xs[1])
    y = root(group, rhs(group, x))
    if y is None:
        return NOT_ON_CURVE, None
    if sign(group, fmt, y) != s:
        y = neg_y(group, y)
    return VALID, (x, y)


def expected_reason(group, fmt, rec):
    return decode(group, fmt, rec)[0]


def is_identity(group, fmt, rec):
    reason, pt = decode(group, fmt, rec)
    return reason == VALID and pt is None


def out_record(group, layout, pt):
    """the decompressed record of a layout; None (identity, and every invalid record) -> the layout's identity encoding"""
    if group == 1:
        return c.g1_rec(layout, pt).encode()
    return c.g2_rec(layout, pt).encode()


def expected_output(group, fmt, layout, recs):
    return b"".join(out_record(group, layout, decode(group, fmt, r)[1]) for r in recs)


def expected_report(group, fmt, recs):
    reasons = bytes(expected_reason(group, fmt, r) for r in recs)
    bad = [i for i, r in enumerate(reasons) if r]
    return {"n_checked": len(recs), "n_invalid": len(bad), "n_identity": sum(is_identity(group, fmt, r) for r in recs),
            "first_invalid": bad[0] if bad else None, "first_reason": reasons[bad[0]] if bad else 0,
            "by_reason": [reasons.count(k) for k in range(5)]}, reasons


def same_report(got, want):
    return {k: got[k] for k in want} == want


def points(group, n, seed):
    return c.g1_points(n, seed) if group == 1 else c.g2_points(n, seed)


def compress_expected(group, fmt, rec: c.Rec):
    """model of the compression of one affine record (a check_ref.Rec): (bytes, bad)"""
    if c.is_identity(rec):
        return encode(group, fmt, None), 0
    if any(v >= P for v in rec.coords):
        return b"\xff" * SIZE[group], 1
    v = [o.fq_from_mont(x) for x in rec.coords]
    pt = (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))
    return encode(group, fmt, pt), 0


# ---- searches (every planted case is found here, by the model) ------------------------------------------------------------
def find_x(group, want_root, seed, norm_nonresidue=False):
    """the first x at or above a seeded start whose right-hand side has (or lacks) a root; G2 with norm_nonresidue: whose
    right-hand side has a NORM without a root"""
    rng = random.Random(seed)
    x = rng.randrange(P // 2) if group == 1 else (rng.randrange(P // 2), rng.randrange(P // 2))
    while True:
        a = rhs(group, x)
        if norm_nonresidue:
            if a[1] and c.sqrt_fq((a[0] * a[0] + a[1] * a[1]) % P) is None:
                return x
        elif (root(group, a) is not None) == want_root:
            return x
        x = x + 1 if group == 1 else (x[0] + 1, x[1])


def nonresidue(seed):
    rng = random.Random(seed)
    a = rng.randrange(2, P)
    while c.sqrt_fq(a) is not None:
        a += 1
    return a


def case_records(group, fmt, seed):
    """(records, names): the planted cases, each record with its name"""
    pts = points(group, 3, seed)
    zero = 0 if group == 1 else (0, 0)
    sflag = flag_bits(fmt, False, 1)
    iflag = flag_bits(fmt, True, 0)
    cases = [("P", encode(group, fmt, pts[0])),
             ("-P", encode(group, fmt, (pts[0][0], neg_y(group, pts[0][1])))),
             ("valid", encode(group, fmt, pts[1])),
             ("identity", encode(group, fmt, None)),
             ("both flag bits", raw_record(group, pts[2][0], 0xC0)),
             ("both flag bits, x = 0", raw_record(group, zero, 0xC0)),
             ("identity flag with bit 0 of x", raw_record(group, 1 if group == 1 else (1, 0), iflag))]
    if group == 1:
        two_g = o.aff_add(o.GEN, o.GEN)
        assert two_g == (0x030644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD3,
                         0x15ED738C0E0A7C92E7845F96B2AE9C0A68A6A449E3538FC7FF3EBF7A5A18A2C4)    # EIP-196 2 G
        cases += [("generator", encode(1, fmt, o.GEN)), ("-generator", encode(1, fmt, o.aff_neg(o.GEN))),
                  ("EIP-196 2 G", encode(1, fmt, two_g)),
                  ("x = p", raw_record(1, P, 0)), ("x = p + 1", raw_record(1, P + 1, sflag)),
                  ("x = 2^254 - 1", raw_record(1, TOP - 1, 0)),
                  ("non-residue right-hand side", raw_record(1, find_x(1, False, seed), 0)),
                  ("non-residue right-hand side, flag set", raw_record(1, find_x(1, False, seed + 1), sflag)),
                  ("x = 0", raw_record(1, 0, 0)), ("x = 0, flag set", raw_record(1, 0, sflag)),
                  ("x = p - 1", raw_record(1, P - 1, 0))]
    else:
        x = pts[2][0]
        sp = c.special_g2()
        cases += [("EIP-197 generator", encode(2, fmt, g.GEN2)), ("-generator", encode(2, fmt, g.neg(g.GEN2))),
                  ("identity flag with a bit of x.c1", raw_record(2, (0, 1 << 200), iflag)),
                  ("c0 = p", raw_record(2, (P, x[1]), 0)), ("c0 = p + 1", raw_record(2, (P + 1, x[1]), sflag)),
                  ("c0 = 2^254 - 1", raw_record(2, (TOP - 1, x[1]), 0)),
                  ("c0 = 2^256 - 1", raw_record(2, ((1 << 256) - 1, x[1]), 0)),
                  ("c1 = p", raw_record(2, (x[0], P), 0)), ("c1 = p + 1", raw_record(2, (x[0], P + 1), sflag)),
                  ("c1 = 2^254 - 1", raw_record(2, (x[0], TOP - 1), 0)),
                  ("right-hand side without a root", raw_record(2, find_x(2, False, seed), 0)),
                  ("right-hand side whose norm is a non-residue", raw_record(2, find_x(2, False, seed, True), sflag)),
                  ("x = 0", raw_record(2, (0, 0), 0)), ("x = (p - 1, 0)", raw_record(2, (P - 1, 0), 0)),
                  ("x = (0, p - 1)", raw_record(2, (0, P - 1), sflag)),
                  ("curve point outside G2", encode(2, fmt, sp["curve"])),
                  ("G2 point + cofactor point", encode(2, fmt, sp["g2_plus_cofactor"]))]
    return [r for _, r in cases], [nm for nm, _ in cases]


def plant(buf: bytes, stride, recs, n, rng):
    """recs at distinct random indices of the n-record array (as many as fit), first and last index included"""
    idx = sorted(rng.sample(range(n), min(n, len(recs))))
    idx[0], idx[-1] = 0, n - 1
    out = bytearray(buf)
    placed = {}
    for i, r in zip(idx, recs):
        out[i * stride:(i + 1) * stride] = r
        placed[i] = r
    return bytes(out), placed


# ---- raw-limb root operands -------------------------------------------------------------------------------------------
def fq_sqrt_operands(seed, n_random=24):
    """(value, lift) pairs: a as the integer a rho + lift p in normalised limbs"""
    rng = random.Random(seed)
    ops = [(0, 0), (1, 0), (P - 1, 0), (4, 0), (4, 1), (4, 3), (P - 1, 3), (nonresidue(seed), 1)]
    ops += [(rng.randrange(P), rng.randrange(4)) for _ in range(n_random)]
    return ops


def fq_sqrt_record(a, lift):
    return g.limbs_of(a * g.RHO % P + lift * P) + [0] * 27


def fq2_sqrt_operands(seed, n_each=64):
    rng = random.Random(seed)
    s, nr, t = rng.randrange(1, P), nonresidue(seed), rng.randrange(1, P)
    a0 = rng.randrange(1, P)
    ops = [(s * s % P, 0), (nr, 0), (0, t * t % P), (0, nonresidue(seed + 1)), (0, 0),
           (a0, 0), (-a0 % P, 0)]            # a1 = 0: n = sqrt(a0^2) is a0 or -a0, one of the two gives a0 + n = 0
    squares, others = [], []
    while len(squares) < n_each or len(others) < n_each:
        a = g.rand_fq2(rng)
        (squares if c.sqrt_fq2(a) is not None else others).append(a)
    return ops + squares[:n_each] + others[:n_each]


def fq2_sqrt_record(a, rng):
    return g.fq2_rec(a, 3, rng) + [0] * 54
