"""Host tests of the term-list sumcheck calls (no GPU): the twins msm_amd_host_fr_sumcheck_round_terms and
msm_amd_host_fr_sumcheck_step_terms against the big-integer model of tests/terms_ref.py, byte for byte; strides and poison;
thread counts; the step in place; every argument error; the degree helper msm_amd_fr_sumcheck_terms_degree; the plan tap
msm_amd_test_fr_sumcheck_terms_plan against the closed form of the round plan."""
import ctypes

import pytest

import mle_ref as m
import terms_ref as t

R = m.R
POISON = b"\xFF" * 32


def tables_of(form, seed, n, layout, stride, edge=False):
    """records of form.n_vec tables, `stride` apart, the gaps filled with 0xEE"""
    if edge:
        return m.pack_raw(m.edge_tables(seed, n, form.n_vec), stride)
    return m.pack([m.random_values(seed + v, n) for v in range(form.n_vec)], layout, stride)


def check_step(step, data, r, layout, order, form, n, stride, tag):
    """a step call into poisoned memory against the model: the n / 2 records of every table, g, and nothing else written"""
    before = POISON * (m.span(n, form.n_vec, stride) + 3)
    out, g = step(data, r, n, order, layout, form.n_vec, stride, out=before)
    exp_tabs, exp_g = t.step(data, r, layout, order, form, n, stride)
    assert m.bind_outputs(out, n, 1, form.n_vec, stride) == exp_tabs, tag
    assert g == exp_g, tag
    assert m.bind_untouched(out, before, n, form.n_vec, stride) is None, tag


@pytest.mark.parametrize("mm", range(1, 9))
def test_twins_match_the_model(msm_pkg, mm):
    n = 1 << mm
    for order in t.ORDERS:
        for layout in t.LAYOUTS:
            for j, form in enumerate(t.FORMS):
                tag = (mm, order, layout, form)
                terms = form.lib_terms(msm_pkg, layout)
                stride = n + 5 * (j & 1)
                data = tables_of(form, 100 * mm + j, n, layout, stride, edge=(j + mm) % 3 == 0)
                assert msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec, stride, threads=3) == \
                    t.round_values(data, layout, order, form, n, stride), tag
                if mm >= 2:
                    r = m.challenges(mm + j, 1, layout, edge=j % 2 == 0)
                    check_step(lambda d, r_, n_, *a, **kw: msm_pkg.host_fr_sumcheck_step_terms(d, r_, n_, terms, *a, threads=3, **kw),
                               data, r, layout, order, form, n, stride, tag)


@pytest.mark.parametrize("form", [t.VANILLA, t.FORMS[6]], ids=repr)
def test_thread_counts_give_the_same_bytes(msm_pkg, form):
    """2^13 records: four ranges of pairs for the round, two for the step's sums"""
    mm, layout = 13, m.MONT_LE
    n = 1 << mm
    terms = form.lib_terms(msm_pkg, layout)
    data = tables_of(form, 13, n, layout, n + 3)
    r = m.challenges(13, 1, layout)
    for order in t.ORDERS:
        rounds = [msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec, n + 3, threads=k) for k in (1, 3, 16)]
        steps = [msm_pkg.host_fr_sumcheck_step_terms(data, r, n, terms, order, layout, form.n_vec, n + 3, threads=k) for k in (1, 3, 16)]
        assert rounds[0] == rounds[1] == rounds[2] and steps[0] == steps[1] == steps[2], order
        if order == t.LOW:
            assert rounds[0] == t.round_values(data, layout, order, form, n, n + 3)
            assert steps[0][1] == t.step(data, r, layout, order, form, n, n + 3)[1]


@pytest.mark.parametrize("mm", [2, 5, 8])
def test_step_high_in_place(msm_pkg, mm):
    n = 1 << mm
    for layout in t.LAYOUTS:
        for form, stride in ((t.VANILLA, n + 5), (t.product(1), n), (t.FORMS[5], n)):
            terms = form.lib_terms(msm_pkg, layout)
            data = tables_of(form, mm, n, layout, stride)
            r = m.challenges(mm, 1, layout)
            out, g = msm_pkg.host_fr_sumcheck_step_terms(data, r, n, terms, t.HIGH, layout, form.n_vec, stride, out="in place")
            exp_tabs, exp_g = t.step(data, r, layout, t.HIGH, form, n, stride)
            assert m.bind_outputs(out, n, 1, form.n_vec, stride) == exp_tabs and g == exp_g, (mm, layout, form)
            assert m.bind_untouched(out, data, n, form.n_vec, stride) is None, (mm, layout, form)


@pytest.mark.parametrize("mm", [1, 4, 7])
def test_lists_that_spell_the_shipped_forms(msm_pkg, mm):
    """PRODUCT of k tables and EQ_AB_C as term lists: the bytes of msm_amd_host_fr_sumcheck_round (outputs are unique)"""
    n = 1 << mm
    for order in t.ORDERS:
        for layout in t.LAYOUTS:
            for form, shipped in [(t.product(k), m.PRODUCT) for k in (1, 2, 3, 4)] + [(t.EQ_AB_C, m.EQ_AB_C)]:
                data = tables_of(form, mm, n, layout, n + 2, edge=True)
                assert msm_pkg.host_fr_sumcheck_round_terms(data, n, form.lib_terms(msm_pkg, layout), order, layout, form.n_vec, n + 2) == \
                    msm_pkg.host_fr_sumcheck_round(data, n, shipped, order, layout, form.n_vec, n + 2), (order, layout, form)


def test_protocol_with_the_model_verifier(msm_pkg):
    """round_terms once, step_terms per challenge, the last variable by mle_eval: every g passes the verifier's step"""
    mm, layout, form = 6, m.CANON_LE, t.GKR
    n0 = 1 << mm
    tabs = [m.random_values(60 + v, n0) for v in range(form.n_vec)]
    coeffs = form.coeff_values(layout)
    terms = form.lib_terms(msm_pkg, layout)
    rs = m.random_values(61, mm)
    point = m.encode(rs, layout)
    for order in t.ORDERS:
        data, n = m.pack(tabs, layout), n0
        claim = t.total(tabs, form, coeffs)
        g = msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec)
        for s in range(mm - 1):
            claim = m.verifier_step(claim, m.decode(g, layout), rs[s])
            out, g = msm_pkg.host_fr_sumcheck_step_terms(data, point[32 * s:32 * s + 32], n, terms, order, layout, form.n_vec, n)
            data, n = b"".join(m.bind_outputs(out, n, 1, form.n_vec, n)), n // 2
        claim = m.verifier_step(claim, m.decode(g, layout), rs[mm - 1])
        finals = m.decode(msm_pkg.host_fr_mle_eval(m.pack(tabs, layout), point, n0, order, layout, form.n_vec), layout)
        assert claim == t.combine(form, coeffs, finals), order


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    one = m.encode([1], m.MONT_LE)
    data = m.pack([m.random_values(v, 16) for v in range(2)], m.MONT_LE)
    out, g = ctypes.create_string_buffer(b"\xA5" * len(data), len(data)), ctypes.create_string_buffer(b"\xA5" * 256, 256)
    ptr = lambda x: None if x is None else ctypes.addressof(x.c)                                          # noqa: E731
    for name, (terms, n, n_vec, stride, order, layout) in t.error_cases(msm_pkg).items():
        assert L.msm_amd_host_fr_sumcheck_round_terms(layout, order, ptr(terms), data, n, n_vec, stride, 0, g) == msm_pkg.INPUT_ERROR, name
        assert L.msm_amd_host_fr_sumcheck_step_terms(layout, order, ptr(terms), one, data, n, n_vec, stride, 0, out, g) == \
            msm_pkg.INPUT_ERROR, name
    good = msm_pkg.SumcheckTerms([(one, [0, 1])])
    rnd = lambda *a: L.msm_amd_host_fr_sumcheck_round_terms(0, 0, ptr(good), *a)                          # noqa: E731
    stp = lambda order, *a: L.msm_amd_host_fr_sumcheck_step_terms(0, order, ptr(good), *a)                # noqa: E731
    buf = ctypes.create_string_buffer(data + data, 2 * len(data))
    at = lambda off: ctypes.c_void_p(ctypes.addressof(buf) + 32 * off)                                    # noqa: E731
    cases = {
        "round: null in": lambda: rnd(None, 16, 2, 16, 0, g), "round: null g_out": lambda: rnd(data, 16, 2, 16, 0, None),
        "step: null r": lambda: stp(0, None, data, 16, 2, 16, 0, out, g), "step: null in": lambda: stp(0, one, None, 16, 2, 16, 0, out, g),
        "step: null out": lambda: stp(0, one, data, 16, 2, 16, 0, None, g), "step: null g_out": lambda: stp(0, one, data, 16, 2, 16, 0, out, None),
        "step: n == 2": lambda: stp(1, one, data, 2, 2, 2, 0, out, g),
        "step: LOW in place": lambda: stp(0, one, at(0), 16, 2, 16, 0, at(0), g),
        "step: LOW partial overlap": lambda: stp(0, one, at(0), 16, 2, 16, 0, at(1), g),
        "step: HIGH partial overlap": lambda: stp(1, one, at(0), 16, 2, 16, 0, at(1), g),
        "step: HIGH output ends inside the input": lambda: stp(1, one, at(8), 16, 2, 16, 0, at(0), g),
        "step: output inside the input span": lambda: stp(1, one, at(0), 16, 2, 16, 0, at(31), g),
    }
    for name, case in cases.items():
        assert case() == msm_pkg.INPUT_ERROR, name
    assert out.raw == b"\xA5" * len(data) and g.raw == b"\xA5" * 256 and buf.raw == data + data    # a refused call writes nothing
    # nothing to do: OK, nothing touched, the list is not looked at
    assert L.msm_amd_host_fr_sumcheck_round_terms(0, 0, None, None, 3, 0, 0, 0, None) == msm_pkg.OK
    assert L.msm_amd_host_fr_sumcheck_step_terms(0, 1, None, None, None, 0, 0, 0, 0, None, None) == msm_pkg.OK
    # right behind the input is disjoint from it, and HIGH may run on the input itself
    assert stp(0, one, at(0), 16, 2, 16, 0, at(32), g) == msm_pkg.OK
    assert stp(1, one, at(0), 16, 2, 16, 0, at(0), g) == msm_pkg.OK


def test_degree_helper(msm_pkg):
    one = m.encode([1], m.MONT_LE)
    for form in t.FORMS:
        assert msm_pkg.sumcheck_terms_degree(form.lib_terms(msm_pkg, m.MONT_LE), form.n_vec) == form.degree, form
        assert msm_pkg.sumcheck_terms_degree(form.lib_terms(msm_pkg, m.MONT_LE), 16) == form.degree, form
    assert max(f.degree for f in t.FORMS) == 7 and min(f.degree for f in t.FORMS) == 1
    L, d = msm_pkg.lib(), ctypes.c_uint32(99)
    for name, (terms, _, n_vec, _, order, layout) in t.error_cases(msm_pkg).items():
        if order == 0 and layout == 0 and name.split()[0] not in ("n", "stride", "n_vec") or name == "n_vec == 17":
            st = L.msm_amd_fr_sumcheck_terms_degree(None if terms is None else ctypes.addressof(terms.c), n_vec, ctypes.byref(d))
            assert st == msm_pkg.INPUT_ERROR and d.value == 99, name
    good = msm_pkg.SumcheckTerms([(one, [0, 1])])
    assert L.msm_amd_fr_sumcheck_terms_degree(ctypes.addressof(good.c), 0, ctypes.byref(d)) == msm_pkg.INPUT_ERROR      # no table
    assert L.msm_amd_fr_sumcheck_terms_degree(ctypes.addressof(good.c), 2, None) == msm_pkg.INPUT_ERROR


def test_plan_tap_against_the_closed_form(msm_pkg):
    P = msm_pkg.test_fr_sumcheck_terms_plan
    for form in (t.product(1), t.VANILLA, t.FORMS[6]):
        terms = form.lib_terms(msm_pkg, m.MONT_LE)
        for chunk_log in (6, 8, 13, 20):
            for mm in (1, 2, 7, 8, 9, 14, 17, 18, 24, 31):
                n = 1 << mm
                if form.n_vec * n >= 1 << 32:
                    continue
                assert P(terms, n, form.n_vec, chunk_log) == t.round_plan(n, form.degree + 1, chunk_log), (form, chunk_log, mm)
                if mm >= 2:
                    assert P(terms, n, form.n_vec, chunk_log, step=True) == t.round_plan(n // 2, form.degree + 1, chunk_log), (form, mm)
    terms = t.VANILLA.lib_terms(msm_pkg, m.MONT_LE)
    # the same plan as the shipped round of as many values, and the geometries the GPU tests rely on
    shipped = msm_pkg.test_fr_mle_plan(msm_pkg.MLE_CALL_ROUND, 1 << 14, 4, form=msm_pkg.SUMCHECK_EQ_AB_C, chunk_log=6)
    assert P(t.EQ_AB_C.lib_terms(msm_pkg, m.MONT_LE), 1 << 14, 4, 6) == shipped
    assert (P(terms, 1 << 7, 9, 6)["launches"], P(terms, 1 << 8, 9, 6)["launches"], P(terms, 1 << 18, 9, 6)["launches"]) == (1, 2, 3)
    assert P(terms, 1 << 14, 9, 6)["first_waves"] == 128 and P(terms, 1 << 2, 9, 6, step=True)["first_waves"] == 1
    for bad in (lambda: P(terms, 1 << 4, 9, 5), lambda: P(terms, 1 << 4, 9, 21), lambda: P(terms, 12, 9), lambda: P(terms, 2, 9, step=True),
                lambda: P(terms, 1 << 4, 8), lambda: P(None, 1 << 4, 9), lambda: P(terms, 1 << 4, 0)):
        with pytest.raises(msm_pkg.MsmError):
            bad()
