"""The lazy Fq12 tower and the pairing steps (csrc/bn254_fq12_29.hip.h) at the edges of their bounds contract, on the host
twin of the device code (msm_amd_test_fq12_ops_host: raw limbs in and out), against the big-integer model: the corpus of
tests/fq12_envelope.py.  Every record's value equals the model, every output is normalised and inside the contract, and
the largest output of every op stays under the figure tools/fq12_bounds.py derives for it (printed: DESIGN.md quotes it)."""
import ctypes
import os
import sys

import pytest

import fq12_envelope as env
import g2_ref as g2
import pairing_ref as pr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fq12_bounds  # noqa: E402

OP_IDS = sorted(env.OP_NAMES)


@pytest.fixture(scope="module")
def figures():
    fq12_bounds.derive()
    return dict(fq12_bounds.FIG)


def run_ops(run, op, recs):
    return env.split(run(op, env.flat(recs, 2), env.flat(recs, 3), len(recs)))


def model_failures(recs, outs):
    return [(r[0], bad) for r, w in zip(recs, outs) if (bad := r[4](w))]


def bound_failures(op, recs, outs):
    return [(r[0], bad) for r, w in zip(recs, outs) if (bad := env.output_failures(op, w))]


def figure_failures(op, outs, figures):
    """the reached maxima against the derived figures; conj has none and is held to the element bound by bound_failures"""
    top = env.reached(op, outs)
    line = ", ".join("%s %.3f p (figure %.3f p)" % (k, top[k], figures[k]) for k, _ in env.GOVERNS[env.OP_NAMES[op]])
    print("\n%-11s largest %.3f p; %s" % (env.OP_NAMES[op], top["largest"], line or "no figure: the element bound, 4 p"))
    return [(k, top[k], figures[k]) for k, _ in env.GOVERNS[env.OP_NAMES[op]] if top[k] > figures[k]]


@pytest.mark.parametrize("op", OP_IDS, ids=[env.OP_NAMES[op] for op in OP_IDS])
def test_op_at_the_bounds(msm_pkg, figures, op):
    recs = env.corpus(op)
    outs = run_ops(msm_pkg.test_fq12_ops_host, op, recs)
    bad = model_failures(recs, outs)
    assert not bad, f"{len(bad)} of {len(recs)} differ from the model, first: {bad[:3]}"
    bad = bound_failures(op, recs, outs)
    assert not bad, f"{len(bad)} of {len(recs)} outside the contract, first: {bad[:3]}"
    over = figure_failures(op, outs, figures)
    assert not over, f"above the derived figure: {over}"


def test_every_class_is_present():
    """the coverage claim as a test: every (op, class) of fq12_envelope.CLAIMED occurs in the corpus, within the sizes"""
    have = {(env.OP_NAMES[op], r[1]) for op in OP_IDS for r in env.corpus(op)}
    print("\n" + ", ".join("%s/%s=%d" % (env.OP_NAMES[op], c, sum(r[1] == c for r in env.corpus(op)))
                           for op in OP_IDS for c in sorted({r[1] for r in env.corpus(op)})))
    missing = sorted(env.CLAIMED - have)
    assert not missing, f"never built: {missing}"
    assert not have - env.CLAIMED, f"built and not claimed: {sorted(have - env.CLAIMED)}"
    for op in OP_IDS:
        assert 0 < len(env.corpus(op)) <= env.MAX_RECORDS.get(op, 400)
    checked = [r for r in env.corpus(pr.FQ12_OP_FINAL_EXP) if r[4] is not env.twin_only]
    assert len(checked) == env.FINAL_EXP_MODEL_CHECKED
    assert sum(r[1].startswith("saturated") for r in checked) == 14        # both saturated forms, the twelve single ones


def test_the_corpus_is_at_the_edge():
    """what the classes promise, checked on the records themselves"""
    sets = env.element_sets()
    sat = env.words_w(sets[0][2])
    assert all(sat[9 * i + k] == env.NLM for i in range(12) for k in range(8))
    assert all(4 * pr.P - (1 << 232) < g2.value(sat[9 * i:9 * i + 9]) <= 4 * pr.P for i in range(12))
    assert 8 * pr.P - (1 << 232) <= g2.value(env.SAT8) < 8 * pr.P
    grid = [c for cls, _, c in sets if cls == "grid"]
    for i in range(12):                                     # every multiple, the top one included, in every position
        assert {c[i] // pr.P for c in grid} == {0, 1, 2, 3}
    zeros = [c for cls, _, c in sets if cls == "edge-zero"]
    assert {c[0] // pr.P for c in zeros if len(set(c)) == 1} == {0, 1, 2, 3, 4}
    forms = [c for cls, _, c in sets if cls == "forms"]
    for k in range(0, len(forms), 3):                       # one value, three limb vectors; the middle one borrows everywhere
        plain, every, some = forms[k:k + 3]
        assert [g2.value(env.limbs(x)) for x in every] == plain == [g2.value(env.limbs(x)) for x in some]
        assert all(l >= 1 << 29 for x in every for l in x[:8]) and every != some
    for op in env.OP_NAMES:
        for r in env.corpus(op):                            # every operand inside its bound, normalised
            assert g2.normalised(r[2], 12) and g2.normalised(r[3], 12), r[0]
            top_b = 8 * pr.P - 1 if op == pr.FQ12_OP_LINE_MUL else pr.P - 1 if env.OP_NAMES[op].endswith("step") else 4 * pr.P
            assert all(g2.value(r[2][9 * i:9 * i + 9]) <= 4 * pr.P for i in range(12)), r[0]
            assert all(g2.value(r[3][9 * i:9 * i + 9]) <= top_b for i in range(12)), r[0]
            if op == pr.FQ12_OP_ADD_STEP:
                assert all(g2.value(r[2][54 + 9 * i:63 + 9 * i]) < pr.P for i in range(2)), r[0]     # Q.x canonical


def test_models_of_the_cyclotomic_maps():
    """gs_sqr and gs_pow_x are the plain square and power on the cyclotomic subgroup (and not elsewhere); the split final
    exponentiation is the plain power"""
    rng = pr.rng_for(77)
    c = pr.rand_cyclotomic(rng)
    assert env.gs_sqr(c) == pr.sqr12(c) and env.gs_pow_x(c) == pr.pow12(c, pr.X_BN)
    a = pr.rand_fq12(rng)
    assert env.gs_sqr(a) != pr.sqr12(a)
    sat = pr.fq12_of(env.words_w(env.element_sets()[0][2]))
    assert env.final_exp_model(sat) == pr.final_exponentiation(sat)


def test_cross_op_identities(msm_pkg):
    """SQR against MUL(a, a) on the same records; CYCLO_SQR against SQR on the cyclotomic records"""
    recs = env.corpus(pr.FQ12_OP_SQR)
    a = env.flat(recs, 2)
    sq = env.split(msm_pkg.test_fq12_ops_host(pr.FQ12_OP_SQR, a, a, len(recs)))
    mu = env.split(msm_pkg.test_fq12_ops_host(pr.FQ12_OP_MUL, a, a, len(recs)))
    assert [pr.fq12_of(w) for w in sq] == [pr.fq12_of(w) for w in mu]
    cyc = [r for r in env.corpus(pr.FQ12_OP_CYCLO_SQR) if r[1] == "cyclo"]
    a = env.flat(cyc, 2)
    cs = env.split(msm_pkg.test_fq12_ops_host(pr.FQ12_OP_CYCLO_SQR, a, a, len(cyc)))
    sq = env.split(msm_pkg.test_fq12_ops_host(pr.FQ12_OP_SQR, a, a, len(cyc)))
    assert len(cyc) >= 30 and [pr.fq12_of(w) for w in cs] == [pr.fq12_of(w) for w in sq]
    inv = [r for r in env.corpus(pr.FQ12_OP_INV) if r[1] != "zero"]
    outs = run_ops(msm_pkg.test_fq12_ops_host, pr.FQ12_OP_INV, inv)
    assert all(pr.mul12(pr.fq12_of(r[2]), pr.fq12_of(w)) == pr.ONE12 for r, w in zip(inv, outs))    # a inv(a) = 1


def test_zero_has_an_answer(msm_pkg):
    """INV and FINAL_EXP of zero (a Miller value that went to zero, at any multiple of p): the spec is only that the call
    returns an element.  What the code gives, and the header says: zero -- Fq2::inv of 0 is 0, and every product after it."""
    for op in (pr.FQ12_OP_INV, pr.FQ12_OP_FINAL_EXP):
        zero = [r for r in env.corpus(op) if r[1] == "zero"]
        assert len(zero) >= 6
        for r, w in zip(zero, run_ops(msm_pkg.test_fq12_ops_host, op, zero)):
            assert env.output_failures(op, w) is None, r[0]
            assert pr.fq12_of(w) == pr.ZERO12, r[0]


def test_add_step_on_opposite_points(msm_pkg):
    """T = Q gives zeros throughout; T = -Q gives the point at infinity (0, Y', 0) with Y' = -theta^3 Z and the vertical
    line (0, -theta x_P, theta x_Q), theta = -2 y_Q Z, not zeros: the division-free step has no exceptional case."""
    recs = env.corpus(pr.FQ12_OP_ADD_STEP)
    outs = run_ops(msm_pkg.test_fq12_ops_host, pr.FQ12_OP_ADD_STEP, recs)
    n = {"step-T=Q": 0, "step-T=-Q": 0}
    for r, w in zip(recs, outs):
        v = [g2.fq2_of(w[18 * k:18 * k + 18]) for k in range(6)]
        if r[1] == "step-T=Q":
            assert v == [pr.ZERO2] * 6, r[0]
        elif r[1] == "step-T=-Q":
            assert v[0] == v[2] == v[3] == pr.ZERO2 and pr.ZERO2 not in (v[1], v[4], v[5]), r[0]
        n[r[1]] = n.get(r[1], 0) + 1
    assert n["step-T=Q"] == 5 == n["step-T=-Q"]


def test_batch_call_arguments(msm_pkg):
    L = msm_pkg.lib()
    n = 3
    recs = env.corpus(pr.FQ12_OP_MUL)[:n]
    a = (ctypes.c_uint32 * (108 * n))(*env.flat(recs, 2))
    b = (ctypes.c_uint32 * (108 * n))(*env.flat(recs, 3))
    out = (ctypes.c_uint32 * (108 * n + 4))(*([0xA5A5A5A5] * (108 * n + 4)))
    fill = list(out)
    for args in ((14, a, b, out, n), (-1, a, b, out, n), (pr.FQ12_OP_MUL, None, b, out, n), (pr.FQ12_OP_MUL, a, None, out, n),
                 (pr.FQ12_OP_MUL, a, b, None, n), (pr.FQ12_OP_MUL, a, b, out, (1 << 20) + 1)):
        assert L.msm_amd_test_fq12_ops_host(*args) == msm_pkg.INPUT_ERROR, args[0]
        assert list(out) == fill
    assert L.msm_amd_test_fq12_ops_host(pr.FQ12_OP_MUL, None, None, None, 0) == msm_pkg.OK       # count = 0 touches nothing
    assert L.msm_amd_test_fq12_ops_host(pr.FQ12_OP_MUL, a, b, out, 0) == msm_pkg.OK and list(out) == fill
    assert L.msm_amd_test_fq12_ops_host(14, None, None, None, 0) == msm_pkg.INPUT_ERROR          # the op is checked first
    assert L.msm_amd_test_fq12_ops_host(pr.FQ12_OP_MUL, a, b, out, n - 1) == msm_pkg.OK
    got = list(out)
    assert got[108 * (n - 1):] == fill[108 * (n - 1):]                                           # nothing behind count records
    assert all(r[4](w) is None for r, w in zip(recs, env.split(got[:108 * (n - 1)])))
    one = msm_pkg.test_fq12_op_host(pr.FQ12_OP_MUL, recs[0][2], recs[0][3])                       # the one-record call forwards
    assert one == got[:108]
    with pytest.raises(ValueError):
        msm_pkg.test_fq12_ops_host(pr.FQ12_OP_MUL, recs[0][2][:-1], recs[0][3], 1 + 1)
    assert msm_pkg.test_fq12_ops_host(pr.FQ12_OP_MUL, [], [], 0) == []
