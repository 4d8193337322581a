"""The lifted subtraction folded into the Montgomery reduction (Fq29::mul_sub_np / sqr_sub_np, bn254_fq29.hip.h:
K - x joins the reduced columns in front of the output carry chain) and the point additions that use it, on the host
twin of the device code (raw-limb ops, no GPU).

  * form equivalence, for every lifted constant K: the folded form returns the value of norm(sub<K>(mul_np(a, b), x)) --
    the product taken from the library's own mul_np / sqr_np, the subtraction and the carry round from the limb-exact
    models of oracle/fq29_ref.py -- and the limbs of the digit-by-digit model of tests/test_fq29_friendly_reduction.py
    with the tail added;
  * the limb contract: limbs 0..7 below 2^29, limb 8 = floor(value / 2^232), inside the bound tools/fq29_bounds.py
    states for the form at the operand limit;
  * operands: random, at the contract's limits (every limb 2^30 + 2^8, value about 40 p; x at the lifted limbs, one
    2^(e-29) below them, at the top-limb headroom, and zero), products equal to x modulo p (the zero filter and the exact
    test must accept the result, from a canonical and from a lazy x), and products whose wide digits overshoot the
    quotient by rho (the + p case);
  * pti_madd, pti_mmadd and pti_add_nz against oracle/bn254_ref.py on the golden point_ops.json cases (a doubling and a
    vanishing sum among them) and over chains of 64 additions that never leave the lazy form."""
import json
import os
import random
import re

import pytest

import test_fq29_eleven_reductions as T
import test_fq29_friendly_reduction as F
from oracle import bn254_ref as o
from oracle import fq29_ref as m

P, MASK = m.P, m.MASK
FE_MUL_SUB, FE_SQR_SUB = 44, 45
KSELS = list(m.KNAMES)                       # the index of a name is the K selector of the raw ops
LIFT_EXP = {k: int(k.split("E")[1]) for k in KSELS}
IN_USE = ("K16E30", "K8E30", "K8E31")        # pti_madd_head's P and R, X3 of every addition
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def raw(msm_pkg, op, recs):
    a = [w for r in recs for w in r[0]]
    b = [w for r in recs for w in r[1]]
    out = msm_pkg.test_op_raw_host(op, a, b, len(recs))
    return [out[m.RAW_OUT * i:m.RAW_OUT * (i + 1)] for i in range(len(recs))]


def fold_record(sel, a, b, x):
    """the raw record of mul_sub_np<sel>(a, b, x); b = None: sqr_sub_np<sel>(a, x)"""
    k = [KSELS.index(sel)] + [0] * 8
    return (m.rec(a, b), m.rec(x, k)) if b is not None else (m.rec(a), m.rec(x, k))


def subtrahends(sel, rng, n):
    """x under sub<K>'s operand contract: the lifted limbs themselves (the most the bounds tool admits, top limb at the
    headroom of K), one 2^(e-29) below them in every limb, zero, the top limb alone, and random ones"""
    K, step = m.KL[sel], 1 << (LIFT_EXP[sel] - 29)
    out = [list(K), [k - step for k in K[:8]] + [K[8]], [0] * 9, [0] * 8 + [K[8]], [k - step for k in K[:8]] + [0]]
    for _ in range(n):
        x = [rng.randint(0, k) if rng.random() < 0.5 else k - rng.randrange(1 << 10) for k in K]
        while m.value(x) > m.KMULT[sel] * P:
            x[8] = rng.randint(0, x[8])
        out.append(x)
    return out


def corpus(sel, square, seed=0, n=40):
    """(a, b or None, x): products at and inside the operand limit against every edge subtrahend, random pairs, and the
    products whose wide digits add up to the canonical quotient + rho"""
    rng = random.Random(9000 + 10 * KSELS.index(sel) + square + seed)
    ops = m.mul_operands(rng, n)                     # the first is every limb at 2^30 + 2^8, value 40 p
    xs = subtrahends(sel, rng, n)
    out = []
    for a, b in list(zip(ops[:7], reversed(ops[:7]))) + [(ops[0], ops[0])]:
        out += [(a, None if square else b, x) for x in xs[:5]]
    out += [(a, None if square else b, x) for a, b, x in zip(ops, reversed(ops), xs)]
    plus_p, _ = F.divergence_corpus("sqr_wide" if square else "mul_wide")   # the module caches it: its own size
    for (ra, rb), x in zip(plus_p[:24], xs):
        out.append((ra[0:9], None if square else rb[0:9], x))
    return out


def check_fold(msm_pkg, sel, recs):
    """violations of the equivalence, the model and the limb contract by the folded form on (a, b or None, x) records"""
    square = recs[0][1] is None
    got = raw(msm_pkg, FE_SQR_SUB if square else FE_MUL_SUB, [fold_record(sel, a, b, x) for a, b, x in recs])
    prod = raw(msm_pkg, T.FE_SQR_WIDE if square else T.FE_MUL_WIDE,
               [(m.rec(a), m.rec(a if square else b)) for a, b, x in recs])
    top_bound = m.FB.contracts()[("sqr_sub<%s>" if square else "mul_sub<%s>") % sel].mx[8]
    K = m.KL[sel]
    bad = []
    for i, ((a, b, x), r, pr) in enumerate(zip(recs, got, prod)):
        r, pr = r[0:9], pr[0:9]
        b = a if square else b
        ref = m.norm(m.sub_limbs(sel, pr, x))        # norm(sub<K>(mul_np(a, b), x)), the form it replaces
        if m.value(r) != m.value(ref):
            bad.append((i, "value differs from norm(sub<K>(mul_np(a, b), x))"))
        if (m.value(r) * m.RHO - m.value(a) * m.value(b) + m.value(x) * m.RHO) % P:
            bad.append((i, "value is not a b / rho - x modulo p"))
        cols = T.columns([(a, b)])
        model = m.canon(m.value(F.friendly_model(cols, True)) + sum((k - y) << (29 * j) for j, (k, y) in enumerate(zip(K, x))))
        if r != model:
            bad.append((i, "limbs differ from the model", r, model))
        if max(r[:8]) > MASK:
            bad.append((i, "limbs 0..7 not below 2^29"))
        if r[8] != m.value(r) >> 232 or r[8] > top_bound:
            bad.append((i, f"top limb {r[8]:#x} outside the tool's bound {top_bound:#x}"))
    return bad, sum(m.value(pr[0:9]) == m.mont(m.value(a) * m.value(a if bb is None else bb)) + P
                    for (a, bb, x), pr in zip(recs, prod))


@pytest.mark.parametrize("square", [False, True], ids=["mul_sub", "sqr_sub"])
@pytest.mark.parametrize("sel", KSELS)
def test_folded_form_equals_the_separate_one(msm_pkg, sel, square):
    recs = corpus(sel, square)
    bad, plus_p = check_fold(msm_pkg, sel, recs)
    assert not bad, f"{len(bad)} of {len(recs)} wrong, first: {bad[:3]}"
    assert plus_p >= 12, "the + p overshoot of the wide digits was not reached"


def test_the_selectors_in_use_are_covered_and_others_give_zero(msm_pkg):
    assert set(IN_USE) <= set(KSELS)
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "metal-msm-gpu-acceleration_amd", "csrc", "bn254_ec29.hip.h")).read()
    assert set(re.findall(r"(?:mul|sqr)_sub_np<(\w+)>", src)) == set(IN_USE)
    one = m.canon(m.to_mont(1))
    r = raw(msm_pkg, FE_MUL_SUB, [(m.rec(one, one), m.rec([0] * 9, [len(KSELS)] + [0] * 8))])[0]
    assert not any(r)


@pytest.mark.parametrize("square", [False, True], ids=["mul_sub", "sqr_sub"])
@pytest.mark.parametrize("sel", IN_USE)
def test_result_zero_modulo_p_passes_the_filter_and_the_exact_test(msm_pkg, sel, square):
    """a b = x (mod p): the result is (k - t) p for x = a b / rho + t p.  x canonical and x lazy (limbs up to 2^30)
    stand for the same value, so both give the same exact limbs; the one-limb filter with the site's bound and the
    exact test accept every one of them, the + p products included."""
    rng = random.Random(77 + KSELS.index(sel) + square)
    k = m.KMULT[sel]
    pairs = [(m.canon(rng.randrange(1, P)), m.canon(rng.randrange(1, P))) for _ in range(24)]
    pairs += [(ra[0:9], rb[0:9]) for ra, rb in F.divergence_corpus("sqr_wide" if square else "mul_wide")[0][:12]]
    prod = raw(msm_pkg, T.FE_SQR_WIDE if square else T.FE_MUL_WIDE, [(m.rec(a), m.rec(a if square else b)) for a, b in pairs])
    recs, want = [], []
    for (a, b), pr in zip(pairs, prod):
        u = m.value(pr[0:9])
        for t in (0, 1, k - 2):
            v = u + t * P
            for x in (m.canon(v), m.spread(v, rng, 1)):
                if v <= k * P and all(y <= kl for y, kl in zip(x, m.KL[sel])):
                    recs.append((a, None if square else b, x))
                    want.append((k - t) * P)
    assert len(recs) >= 100
    got = raw(msm_pkg, FE_SQR_SUB if square else FE_MUL_SUB, [fold_record(sel, a, b, x) for a, b, x in recs])
    assert [m.value(r[0:9]) for r in got] == want
    assert all(r[0:9] == m.canon(v) for r, v in zip(got, want))
    flags = raw(msm_pkg, m.FE_ZERO, [(m.rec(r[0:9]), m.rec([k + 1] + [0] * 8)) for r in got])
    assert all(f[0:2] == [1, 1] for f in flags)


# ---- the point additions ---------------------------------------------------------------------------------------------
def golden_pairs():
    with open(os.path.join(GOLDEN, "point_ops.json")) as f:
        g = json.load(f)

    def pt(v):
        return None if v is None else (int(v[0], 16), int(v[1], 16))
    return [(pt(c["p"]), pt(c["q"]), pt(c["sum"])) for c in g["add"]]


def point_records(op, p, q, rng, wide_neg):
    """raw (a, b) of one addition p + q: p an XYZZ point at the invariant's edge (pti_mmadd: an affine base with a
    normalised y), q a base (y plain or lazily negated) or, for pti_add_nz, another XYZZ point"""
    if op == m.PT_MMADD:
        px, py = m.affine_base(p, wide_neg)
        a = m.rec(px, m.norm(py))
    else:
        a = m.rec(*m.xyzz(p, rng))
    b = m.rec(*m.xyzz(q, rng)) if op == m.PT_ADD_NZ else m.rec(*m.affine_base(q, not wide_neg))
    return a, b


@pytest.mark.parametrize("op", [m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ], ids=["pti_madd", "pti_mmadd", "pti_add_nz"])
def test_point_additions_on_the_golden_cases(msm_pkg, op):
    rng = random.Random(300 + op)
    cases = [(p, q, s) for p, q, s in golden_pairs() if p is not None and q is not None]
    assert any(p == q for p, q, _ in cases) and any(s is None for _, _, s in cases)     # a doubling, a vanishing sum
    recs, exp = [], []
    for i, (p, q, s) in enumerate(cases):
        for wide_neg in (False, True):
            recs.append(point_records(op, p, q, rng, wide_neg))
            exp.append(s)
    outs = raw(msm_pkg, op, recs)
    classes = [m.classify(op, a, b) for a, b in recs]
    bad = [(i, cls, v) for i, ((a, b), r, s, cls) in enumerate(zip(recs, outs, exp, classes))
           if (v := m.point_check(op, a, b, r, s, cls))]
    assert not bad, bad[:3]
    assert {"generic", "double", "vanish"} <= {c[0] for c in classes}


@pytest.mark.parametrize("op", [m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ], ids=["pti_madd", "pti_mmadd", "pti_add_nz"])
def test_chain_of_64_additions_stays_inside_the_invariant(msm_pkg, op):
    """Every result re-enters as the next accumulator with the limbs it came out with (no conversion in between): the
    lazy bounds across iterations.  pti_mmadd starts the chain (affine + affine) and pti_madd carries it on, as the
    accumulate kernel does; the addends repeat, so the chain passes through a doubling (acc == q) and restarts after a
    vanishing sum (acc == -q)."""
    rng = random.Random(640 + op)
    pts = [o.scalar_mul(rng.randrange(1, o.R_ORDER), o.GEN) for _ in range(6)]
    first = pts[0]
    addends = [pts[1 + i % 5] for i in range(60)]
    acc = o.aff_add(first, pts[1])
    addends[0] = pts[1]
    addends[1] = acc                                   # acc + acc: the doubling inside a chain
    addends[2] = o.aff_neg(o.aff_add(acc, acc))        # then its negative: the sum vanishes
    addends += [pts[2], pts[3], pts[3], pts[4]]        # 64 additions in all
    assert len(addends) == 64
    a, acc = None, first
    for i, q in enumerate(addends):
        if acc is None:                                # the identity: the kernels restart from the addend
            a, acc = None, q
            continue
        step_op = op if a is None or op != m.PT_MMADD else m.PT_MADD
        if a is None:
            ra, rb = point_records(step_op, acc, q, rng, i % 2 == 0)
        else:
            rb = m.rec(*m.xyzz(q, rng)) if step_op == m.PT_ADD_NZ else m.rec(*m.affine_base(q, i % 2 == 0))
            ra = a
        out = raw(msm_pkg, step_op, [(ra, rb)])[0]
        want = o.aff_add(acc, q)
        bad = m.point_check(step_op, ra, rb, out, want, m.classify(step_op, ra, rb))
        assert not bad, (i, bad)
        acc = want
        a = out[0:36] + [0] * (m.RAW_IN - 36) if want is not None else None
    assert acc == o.msm_naive([1] * 65, [first] + addends)
