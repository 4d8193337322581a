"""The point additions' wide quotient digits (Fq29::reduce_columns<true>: digits 0..7 unmasked) and the full addition
in 11 reductions (pti_add_nz), on the host twin and on the device, against big-integer models written here.

oracle/fq29_ref.py models the masked reduction and today's textbook grouping of the full addition; this file adds
  * reduce_model: reduce_columns digit by digit from the 17 column sums, masked or wide, asserting that no column
    reaches 2^64 -- the exact limbs the code must return;
  * add_nz_model: P = X2 ZZ1 - X1 ZZ2 and R = Y2 ZZZ1 - Y1 ZZZ2 as wide double products, the bound-2 filter on P,
    V = ZZ2 PP, Tz = ZZZ2 PPP, Q = X1 V, ZZ3 = ZZ1 V, ZZZ3 = ZZZ1 Tz, Y3 = R (Q - X3) - Y1 Tz (masked)."""
import collections
import random

import pytest

from oracle import fq29_ref as m
from test_host_fq29_envelope import run_raw

P = m.P
PL = m.PL
INV29 = 0x04866389            # -p^-1 mod 2^29, the header's Fq29::INV
U64 = 1 << 64
NORM_MAX = m.NORM_LIMB_MAX
FE_MUL_WIDE, FE_SQR_WIDE, FE_MUL2_WIDE = 32, 33, 34
WIDE_NAMES = {FE_MUL_WIDE: "FE_MUL_WIDE", FE_SQR_WIDE: "FE_SQR_WIDE", FE_MUL2_WIDE: "FE_MUL2_WIDE"}


# ---- models --------------------------------------------------------------------------------------------------------
def columns(pairs):
    cols = [0] * 17
    for a, b in pairs:
        for i in range(9):
            for j in range(9):
                cols[i + j] += a[i] * b[j]
    for c in cols:
        assert c < U64, "a product column reaches 2^64 before the reduction"
    return cols


def reduce_model(cols, wide):
    """reduce_columns<wide> on exact integers; asserts that every intermediate column stays below 2^64"""
    A = list(cols)
    carry = 0
    for k in range(9):
        A[k] += carry
        d = ((A[k] & 0xFFFFFFFF) * INV29) & 0xFFFFFFFF
        if not (wide and k < 8):
            d &= m.MASK
        for j in range(9):
            A[k + j] += d * PL[j]
            assert A[k + j] < U64, f"column {k + j} reaches 2^64 during the reduction"
        assert A[k] & m.MASK == 0
        carry = A[k] >> 29
    r = []
    for k in range(9, 17):
        A[k] += carry
        assert A[k] < U64
        r.append(A[k] & m.MASK)
        carry = A[k] >> 29
    return r + [carry & 0xFFFFFFFF]


def red(pairs, wide=True):
    return reduce_model(columns(pairs), wide)


def add_limbs(a, b):
    return [x + y for x, y in zip(a, b)]


def sub_checked(sel, a, b):
    r = m.sub_limbs(sel, a, b)
    assert all(0 <= x < 1 << 32 for x in r), f"sub<{sel}> leaves 32 bits"
    return r


def add_nz_model(a, b):
    """(branch, j, result limbs or None) of pti_add_nz on raw records a, b; result None for the doubling (its limbs
    are pti_double's, checked through the decoded point)"""
    X1, Y1, ZZ1, ZZZ1 = (a[9 * i:9 * i + 9] for i in range(4))
    X2, Y2, ZZ2, ZZZ2 = (b[9 * i:9 * i + 9] for i in range(4))
    Pl = red([(X2, ZZ1), (X1, m.neg_wide(ZZ2))])
    Rl = red([(Y2, ZZZ1), (Y1, m.neg_wide(ZZZ2))])
    assert m.value(Pl) < 1.40 * P and m.value(Rl) < 1.21 * P
    if m.maybe_zero(Pl[0], 2):
        j = m.filter_multiple(m.value(Pl))
        if j is not None:
            if m.value(Rl) % P == 0:
                return "double", j, None
            one = m.canon(m.to_mont(1))
            return "vanish", j, one + one + [0] * 18
        branch = "filter_pass"
    else:
        branch = "generic"
    PP = red([(Pl, Pl)])
    PPP = red([(Pl, PP)])
    V = red([(ZZ2, PP)])
    Tz = red([(ZZZ2, PPP)])
    Q = red([(X1, V)])
    RR = red([(Rl, Rl)])
    X3 = m.norm(sub_checked("K8E31", RR, add_limbs(PPP, add_limbs(Q, Q))))
    T = sub_checked("K16E30", Q, X3)
    Y3 = red([(Rl, T), (Y1, m.neg_wide(Tz))], wide=False)
    ZZ3 = red([(ZZ1, V)])
    ZZZ3 = red([(ZZZ1, Tz)])
    return branch, None, X3 + Y3 + ZZ3 + ZZZ3


# ---- wide-digit field corpus ---------------------------------------------------------------------------------------
def _norm_at_max(vmax):
    low = [NORM_MAX] * 8
    return low + [m.top_for(low, vmax)]


def _norm_rand(rng, vmax):
    return m._rand_limbs(rng, NORM_MAX, vmax)


def _plus_p_operand(rng, other, partial, vmax):
    """b with partial + other * b = -p * M (mod rho) for a small M: the masked quotient is M, so the wide digits add up
    to M + rho and the result is the masked one + p (the rare case).  None when b would leave [0, vmax)."""
    inv = pow(m.value(other), -1, m.RHO)
    M = rng.randrange(1, 1 << 20)
    b = ((-P * M - partial) * inv) % m.RHO
    return m.canon(b) if b < vmax else None


def wide_corpus(op, seed=0, n=200):
    """raw (a, b) records: operands at the column-sum extremes of the contract (mul / sqr: oracle/fq29_ref.py's
    mul_operands; mul2: pti_add_nz's P = X2 ZZ1 + X1 (-ZZ2) with every limb at its maximum), random ones, and
    constructed products whose wide digits sum to m + rho"""
    rng = random.Random(4242 + 100 * op + seed)
    if op in (FE_MUL_WIDE, FE_SQR_WIDE):
        ops = m.mul_operands(rng, n)
        out = [(m.rec(x), m.rec(y)) for x, y in zip(ops, reversed(ops))] + [(m.rec(x), m.rec(x)) for x in ops[:8]]
        if op == FE_MUL_WIDE:
            while len(out) < len(ops) + 8 + 64:
                a = m.canon(rng.randrange(1, P) | 1)
                b = _plus_p_operand(rng, a, 0, m.MUL_VALUE_MAX)
                if b is not None:
                    out.append((m.rec(a), m.rec(b)))
        return out
    if op == FE_MUL2_WIDE:
        x_max, zz_max = 10 * P, 28 * P // 10
        out = [(m.rec(_norm_at_max(x_max), _norm_at_max(zz_max)), m.rec(_norm_at_max(x_max), list(m.KL["K4E30"]))),
               (m.rec(_norm_at_max(x_max), _norm_at_max(zz_max)), m.rec(_norm_at_max(x_max), m.neg_wide([0] * 9)))]
        for _ in range(n):
            out.append((m.rec(_norm_rand(rng, x_max), _norm_rand(rng, zz_max)),
                        m.rec(_norm_rand(rng, x_max), m.neg_wide(_norm_rand(rng, zz_max)))))
        added = 0
        while added < 64:
            a0, a1 = m.canon(rng.randrange(P)), m.canon(rng.randrange(P))
            b0 = m.canon(rng.randrange(1, P) | 1)
            b1 = _plus_p_operand(rng, b0, m.value(a0) * m.value(a1), 4 * P)
            if b1 is not None and all(x <= k for x, k in zip(b1, m.KL["K4E30"])):
                out.append((m.rec(a0, a1), m.rec(b0, b1)))
                added += 1
        return out
    raise ValueError(op)


def wide_sum(op, a, b):
    a0, a1, b0, b1 = a[0:9], a[9:18], b[0:9], b[9:18]
    if op == FE_MUL_WIDE:
        return [(a0, b0)]
    if op == FE_SQR_WIDE:
        return [(a0, a0)]
    return [(a0, a1), (b0, b1)]


def wide_failures(op, corpus, outs):
    """violations, and how many results took the + p"""
    bad, plus_p = [], 0
    for i, ((a, b), r) in enumerate(zip(corpus, outs)):
        pairs = wide_sum(op, a, b)
        s = sum(m.value(x) * m.value(y) for x, y in pairs)
        exp = reduce_model(columns(pairs), wide=True)
        got = r[0:9]
        if got != exp:
            bad.append((i, "limbs differ from the wide-digit model", got, exp))
        v = m.value(got)
        if v == m.mont(s) + P:
            plus_p += 1
        elif v != m.mont(s):
            bad.append((i, "value is neither mont(s) nor mont(s) + p"))
        if max(got[:8]) > m.MASK:
            bad.append((i, "limbs 0..7 not below 2^29"))
        if any(r[9:]):
            bad.append((i, "words beyond the result are not zero"))
    return bad, plus_p


# ---- point corpus --------------------------------------------------------------------------------------------------
def add_corpus(op, seeds=(0, 1)):
    """oracle/fq29_ref.py's point corpus of pti_add_nz / pti_add (random, equal, opposite partners at the invariant's
    edges: lifted coordinates, borrowed limbs, X / ZZ limbs at the normalised maximum), for two seeds"""
    out = []
    for seed in seeds:
        out += [(a, b, exp) for a, b, exp, _cls in m.point_corpus(op, seed=seed)]
    return out


def add_failures(op, corpus, outs):
    bad, reached = [], collections.Counter()
    for i, ((a, b, exp), r) in enumerate(zip(corpus, outs)):
        ident_a, ident_b = not any(a[18:27]), not any(b[18:27])
        try:
            got = m.decode_point(r[0:36])
        except AssertionError as e:
            bad.append((i, f"not a valid XYZZ point: {e}"))
            continue
        if got != exp:
            bad.append((i, "sum differs from the oracle's"))
        bad += [(i, v) for v in m.point_post(r[0:36])]
        if op == m.PT_ADD and (ident_a or ident_b):
            want = b if ident_a else a
            if r[0:36] != want[0:36]:
                bad.append((i, "identity operand: the other operand does not come back unchanged"))
            continue
        branch, j, limbs = add_nz_model(a, b)
        reached[(branch, j)] += 1
        if limbs is not None and r[0:36] != limbs:
            bad.append((i, f"limbs differ from the 11-reduction model ({branch})"))
        want_flag = int(branch == "vanish") if op == m.PT_ADD_NZ else 0
        if r[36] != want_flag:
            bad.append((i, f"vanished = {r[36]} for branch {branch}"))
        if any(r[37:]):
            bad.append((i, "words beyond the result are not zero"))
    return bad, reached


# ---- host twin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(WIDE_NAMES), ids=list(WIDE_NAMES.values()))
def test_wide_digit_reduction_at_the_bounds(msm_pkg, op):
    corpus = wide_corpus(op)
    outs = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    bad, plus_p = wide_failures(op, corpus, outs)
    print(f"\n{WIDE_NAMES[op]}: {len(corpus)} records, {plus_p} took the + p")
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"
    if op != FE_SQR_WIDE:
        assert plus_p > 0, "no constructed record reached the m + rho case"


@pytest.mark.parametrize("op", [m.PT_ADD_NZ, m.PT_ADD], ids=["PT_ADD_NZ", "PT_ADD"])
def test_full_addition_in_eleven_reductions(msm_pkg, op):
    corpus = add_corpus(op)
    outs = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    bad, reached = add_failures(op, corpus, outs)
    print(f"\n{m.OP_NAMES[op]}: reached " + ", ".join(f"{k}={v}" for k, v in sorted(reached.items(), key=str)))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"
    # P < 1.40 p: a multiple of p is p itself (P = 0 would need both products zero), inside the bound-2 filter
    assert {("double", 1), ("vanish", 1), ("generic", None)} <= set(reached)
    assert not {k for k in reached if k[0] in ("double", "vanish") and k[1] != 1}


# ---- device: the same corpora, bit-exact with the host twin ---------------------------------------------------------
def _device_vs_host(cfg, msm_pkg, op, corpus):
    dev = run_raw(cfg.test_op_raw, op, corpus)
    host = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    diff = [i for i, (d, h) in enumerate(zip(dev, host)) if d != h]
    assert not diff, f"device and host twin differ in {len(diff)} records, first {diff[:5]}"
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(WIDE_NAMES), ids=list(WIDE_NAMES.values()))
def test_wide_digit_reduction_device(cfg, msm_pkg, op):
    corpus = wide_corpus(op)
    bad, _plus_p = wide_failures(op, corpus, _device_vs_host(cfg, msm_pkg, op, corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


@pytest.mark.gpu
@pytest.mark.parametrize("op", [m.PT_ADD_NZ, m.PT_ADD], ids=["PT_ADD_NZ", "PT_ADD"])
def test_full_addition_in_eleven_reductions_device(cfg, msm_pkg, op):
    corpus = add_corpus(op)
    bad, reached = add_failures(op, corpus, _device_vs_host(cfg, msm_pkg, op, corpus))
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"
    assert {("double", 1), ("vanish", 1), ("generic", None)} <= set(reached)


def test_unknown_raw_ops_stay_refused(msm_pkg):
    rec = [0] * m.RAW_IN
    for op in (20, 31, 35):
        with pytest.raises(msm_pkg.MsmError):
            msm_pkg.test_op_raw_host(op, rec, rec, 1)
