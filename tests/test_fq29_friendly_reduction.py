"""Fq29::reduce_columns with quotient digits 0..6 taken straight from the column (reduction by N = INVF p = -1 mod 2^29,
no multiplication by INV; digits 7 and 8 classic), on the host twin and on the device, against a digit-by-digit
big-integer model written here.

  * friendly_model: the 17 column sums through the new reduction, wide (low 32 bits of the column, carry 8 * hi32) or
    masked (low 29 bits, carry column >> 29), asserting that no column reaches 2^64 -- the exact limbs the code returns;
  * the corpora of the earlier reduction tests (oracle/fq29_ref.py, tests/test_fq29_eleven_reductions.py), on which the
    classic and the new form agree, and a constructed one on which they do NOT: products whose canonical quotient is so
    small that the new digits overshoot it by rho and the classic ones do not (the result is then the classic one + p,
    or, rarely, the other way round);
  * the point additions built on it (device = host twin, affine sum = the oracle's) and one whole MSM."""
import random

import pytest

import test_fq29_eleven_reductions as T
from oracle import bn254_ref as o
from oracle import c_oracle as co
from oracle import fq29_ref as m
from test_host_fq29_envelope import point_failures, run_raw

P, RHO, MASK, U64 = m.P, m.RHO, m.MASK, 1 << 64
INV29, PL = T.INV29, m.PL
FRIENDLY_DIGITS = 7
T_BEST = 2
INVF = INV29 + (T_BEST << 29)
NPP_VALUE = (INVF * P + 1) >> 29
NPP = [(NPP_VALUE >> (29 * i)) & MASK for i in range(9)]

# name -> (raw op, wide digits) -- the wide ops are the point additions' forms (mul_np, sqr_np, mul2w_np),
# the masked ones Fq29::mul / mul2 as every other caller (G2's Fq2, the conversions, mul2_np) uses them
OPS = {"mul_wide": (T.FE_MUL_WIDE, True), "sqr_wide": (T.FE_SQR_WIDE, True), "mul2_wide": (T.FE_MUL2_WIDE, True),
       "mul_masked": (m.FE_MUL, False), "mul2_masked": (m.FE_MUL2, False)}


# ---- model -----------------------------------------------------------------------------------------------------------
def friendly_model(cols, wide):
    """reduce_columns<wide> on exact integers, digit by digit; every column is checked against 2^64 when it is read"""
    A = list(cols)
    for k in range(FRIENDLY_DIGITS):
        assert A[k] < U64, f"column {k} reaches 2^64 during the reduction"
        d = A[k] & (0xFFFFFFFF if wide else MASK)
        for j in range(9):
            A[k + 1 + j] += d * NPP[j]
        A[k + 1] += (A[k] >> 32) * 8 if wide else A[k] >> 29
    carry = 0
    for k in range(FRIENDLY_DIGITS, 9):
        A[k] += carry
        d = ((A[k] & 0xFFFFFFFF) * INV29) & 0xFFFFFFFF
        if not (wide and k < 8):
            d &= MASK
        for j in range(9):
            A[k + j] += d * PL[j]
        assert A[k] < U64, f"column {k} reaches 2^64 during the reduction"
        assert A[k] & MASK == 0
        carry = A[k] >> 29
    r = []
    for k in range(9, 17):
        A[k] += carry
        assert A[k] < U64, f"column {k} reaches 2^64"
        r.append(A[k] & MASK)
        carry = A[k] >> 29
    assert carry < 1 << 32
    return r + [carry]


def pairs_of(name, a, b):
    a0, a1, b0, b1 = a[0:9], a[9:18], b[0:9], b[9:18]
    if name in ("mul_wide", "mul_masked"):
        return [(a0, b0)]
    if name == "sqr_wide":
        return [(a0, a0)]
    return [(a0, a1), (b0, b1)]


def failures(name, corpus, outs):
    """violations of the model and of the stated result (mont(s) or mont(s) + p, limbs 0..7 below 2^29), and how many
    records took the + p"""
    wide = OPS[name][1]
    bad, plus_p = [], 0
    for i, ((a, b), r) in enumerate(zip(corpus, outs)):
        pairs = pairs_of(name, a, b)
        s = sum(m.value(x) * m.value(y) for x, y in pairs)
        exp = friendly_model(T.columns(pairs), wide)
        got = r[0:9]
        if got != exp:
            bad.append((i, "limbs differ from the model", got, exp))
        v = m.value(got)
        if v == m.mont(s) + P:
            plus_p += 1
        elif v != m.mont(s):
            bad.append((i, "value is neither mont(s) nor mont(s) + p"))
        if v * RHO >= s + P * RHO * (1 + (2.0 ** -24 if wide else 2.0 ** -27)):
            bad.append((i, "value above s / rho + p (1 + 2^-24) (masked: 2^-27)"))
        if max(got[:8]) > MASK:
            bad.append((i, "limbs 0..7 not below 2^29"))
        if any(r[9:]):
            bad.append((i, "words beyond the result are not zero"))
    return bad, plus_p


# ---- corpora ---------------------------------------------------------------------------------------------------------
def shared_corpus(name):
    """the records of the earlier tests: operands at the column extremes of the contracts, random ones, and the
    constructed products whose wide digits sum to the canonical quotient + rho"""
    op = OPS[name][0]
    return T.wide_corpus(op) if OPS[name][1] else m.field_corpus(op)


def _sqrt_mod_rho(c):
    """x with x^2 = c (mod rho) for c = 1 (mod 8), the root below 2^259 (Hensel: a root mod 2^k lifts to one mod 2^(k+1))"""
    x = 1
    for k in range(3, 261):
        if (x * x - c) >> k & 1:
            x += 1 << (k - 1)
    assert (x * x - c) % RHO == 0
    x %= 1 << 260
    return min(x, (1 << 260) - x)


def _candidate(name, rng, qbits):
    """one record whose product sum is -p Q (mod rho) for a canonical quotient Q below 2^qbits, as _plus_p_operand of the
    earlier tests builds them; None when the solved operand leaves the op's contract"""
    Q = rng.randrange(1, 1 << qbits)
    if name == "sqr_wide":
        Q = (Q & ~7) | (-pow(P, -1, 8) % 8)          # -p Q = 1 (mod 8): an odd square
        a = _sqrt_mod_rho(-P * Q % RHO)
        return (m.rec(m.canon(a)), m.rec([0] * 9)) if a < m.MUL_VALUE_MAX else None
    if name in ("mul_wide", "mul_masked"):
        a = m.canon(rng.randrange(1, P) | 1)
        b = (-P * Q) * pow(m.value(a), -1, RHO) % RHO
        return (m.rec(a), m.rec(m.canon(b))) if b < m.MUL_VALUE_MAX else None
    a0, a1 = m.canon(rng.randrange(P)), m.canon(rng.randrange(P))
    b0 = m.canon(rng.randrange(1, P) | 1)
    b1 = (-P * Q - m.value(a0) * m.value(a1)) * pow(m.value(b0), -1, RHO) % RHO
    if name == "mul2_wide":      # pti_add_nz's P: the fourth operand is a neg_wide value, below 4 p inside the K4E30 limbs
        ok = b1 < 4 * P and all(x <= k for x, k in zip(m.canon(b1), m.KL["K4E30"]))
    else:                        # Fq2's double products: four normalised operands below 64 p
        ok = b1 < 64 * P
    return (m.rec(a0, a1), m.rec(b0, m.canon(b1))) if ok else None


_divergent = {}


def divergence_corpus(name, want=72):
    """records (fixed seed) on which the classic model (tests/test_fq29_eleven_reductions.py reduce_model) and the new one
    return different limbs.  The new digits 0..7 add up to less than 2^236.7 (wide; 2^233.7 masked), the classic wide
    ones to less than 2^235.2, the classic masked ones to the quotient itself: the forms part where the quotient lies
    between the two sums, hence the range the quotients are drawn from."""
    if name not in _divergent:
        wide = OPS[name][1]
        rng = random.Random(29_000 + sorted(OPS).index(name))
        out, tried = [], 0
        while len(out) < want:
            c = _candidate(name, rng, 237 if wide else 233)
            if c is None:
                continue
            tried += 1
            cols = T.columns(pairs_of(name, *c))
            if T.reduce_model(cols, wide) != friendly_model(cols, wide):
                out.append(c)
        _divergent[name] = (out, tried)
    return _divergent[name]


# ---- the model itself ------------------------------------------------------------------------------------------------
def test_constants_and_their_derivation(msm_pkg):
    assert (INVF * P + 1) % (1 << 29) == 0 and NPP_VALUE >> 261 == 0
    sums = {t: sum((((INV29 + (t << 29)) * P + 1) >> 29 >> (29 * i)) & MASK for i in range(9)) for t in range(64)}
    assert all((((INV29 + (t << 29)) * P + 1) >> 29) >> 261 == 0 for t in range(64))
    assert min(sums, key=sums.get) == T_BEST and sums[T_BEST] == 1_028_434_108 < sum(PL)
    # the header's table and digit count, as tools/fq29_bounds.py reads them
    assert m.FB.NPP == NPP and m.FB.INVF == INVF and m.FB.FRIENDLY_DIGITS == FRIENDLY_DIGITS
    # digits 0..7 at their maxima stay below 2^-24 rho (wide) / 2^-27 rho (masked): what the result bound rests on
    for wide, lim in ((True, -24), (False, -27)):
        d = [0xFFFFFFFF if wide else MASK] * 8
        t = sum(d[k] * INVF << (29 * k) for k in range(7)) + (d[7] << 203)
        assert t < RHO * 2.0 ** lim
        assert m.FB.EXTRA[wide] < 2.0 ** lim


@pytest.mark.parametrize("name", list(OPS))
def test_model_agrees_with_the_classic_one_on_the_shared_corpora(name):
    """why the earlier limb-pinning tests still hold: on their fixed corpora both forms return the same limbs"""
    wide = OPS[name][1]
    for a, b in shared_corpus(name):
        cols = T.columns(pairs_of(name, a, b))
        assert friendly_model(cols, wide) == T.reduce_model(cols, wide)


# ---- host twin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPS))
def test_raw_ops_equal_the_model_host(msm_pkg, name):
    corpus = shared_corpus(name)
    assert len(corpus) >= 200
    bad, plus_p = failures(name, corpus, run_raw(msm_pkg.test_op_raw_host, OPS[name][0], corpus))
    print(f"\n{name}: {len(corpus)} records, {plus_p} took the + p")
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


@pytest.mark.parametrize("name", list(OPS))
def test_divergence_corpus_host(msm_pkg, name):
    corpus, tried = divergence_corpus(name)
    print(f"\n{name}: {len(corpus)} of {tried} candidates part the two forms")
    assert len(corpus) >= 64
    bad, plus_p = failures(name, corpus, run_raw(msm_pkg.test_op_raw_host, OPS[name][0], corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"
    assert plus_p > 0


@pytest.mark.parametrize("op", [m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ, m.PT_ADD], ids=lambda op: m.OP_NAMES[op])
def test_point_additions_host(msm_pkg, op):
    corpus = m.point_corpus(op)
    bad = point_failures(op, corpus, run_raw(msm_pkg.test_op_raw_host, op, corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


# ---- device ----------------------------------------------------------------------------------------------------------
def _device_and_host(cfg, msm_pkg, op, corpus):
    dev = run_raw(cfg.test_op_raw, op, corpus)
    host = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    diff = [i for i, (d, h) in enumerate(zip(dev, host)) if d != h]
    assert not diff, f"device and host twin differ in {len(diff)} records, first {diff[:5]}"
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPS))
def test_raw_ops_equal_the_model_device(cfg, msm_pkg, name):
    corpus = shared_corpus(name) + divergence_corpus(name)[0]
    bad, plus_p = failures(name, corpus, _device_and_host(cfg, msm_pkg, OPS[name][0], corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"
    assert plus_p > 0


@pytest.mark.gpu
@pytest.mark.parametrize("op", [m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ, m.PT_ADD], ids=lambda op: m.OP_NAMES[op])
def test_point_additions_device(cfg, msm_pkg, op):
    corpus = m.point_corpus(op)
    bad = point_failures(op, corpus, _device_and_host(cfg, msm_pkg, op, corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


# ---- one whole MSM ---------------------------------------------------------------------------------------------------
def _msm_instance(n=1 << 12):
    """2^12 bases with the exceptional cases inside: a base twice under one scalar (doubling in every window), a base and
    its negative under one scalar (the bucket vanishes), both followed by a third base of the same bucket, an identity
    record, and the scalars 0, 1, r - 1"""
    pts, _ = co.gen_instance(o.SEED_BASE + 2900, n)
    rng = random.Random(2900)
    ks = [rng.randrange(o.R_ORDER) for _ in range(n)]
    recs = [pts[64 * i:64 * i + 64] for i in range(n)]
    x, y = (o.fq_from_mont(int.from_bytes(recs[20][i:i + 32], "little")) for i in (0, 32))
    recs[11] = recs[10]
    ks[11] = ks[12] = ks[10]
    recs[21] = o.encode_affine_h2c(o.aff_neg((x, y)))
    ks[21] = ks[22] = ks[20]
    recs[30] = bytes(64)
    ks[40], ks[41], ks[42] = 0, 1, o.R_ORDER - 1
    return ks, b"".join(recs)


@pytest.mark.gpu
def test_whole_msm_parity_shipped_and_small_window(cfg, msm_pkg):
    ks, pts = _msm_instance()
    n = len(ks)
    sc = b"".join(o.encode_scalar_h2c(k) for k in ks)
    want = o.decode_jacobian_mont_le(co.msm_best(sc, pts, n, 2))
    ds, dp = cfg.alloc(len(sc)), cfg.alloc(len(pts))
    try:
        cfg.to_device(ds, sc)
        cfg.to_device(dp, pts)
        for c in (0, 7):
            cfg.set_window_size(c)
            out = cfg.msm_batch_device([ds], [dp], [n])[0]
            assert o.decode_jacobian_mont_le(out) == want, f"window {c or 'shipped'}"
    finally:
        cfg.set_window_size(0)
        cfg.free(ds)
        cfg.free(dp)
