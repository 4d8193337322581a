"""Host tests of the gate polynomials (no GPU): the twin msm_amd_host_fr_gate_eval against the big-integer model of
tests/gate_ref.py, byte for byte, on the shapes the GPU tests use; accumulate and scale; poison; thread counts; every refusal
of msm_amd_fr_gate_check and of the call, by text; the plan tap msm_amd_test_fr_gate_plan on hand-worked term lists."""
import ctypes

import pytest

import gate_ref as g
import mle_ref as m

R = g.R
POISON = b"\xFF" * 32


@pytest.mark.parametrize("n", g.SIZES)
def test_twin_matches_the_model(msm_pkg, n):
    for layout in g.LAYOUTS:
        for j, gate in enumerate(g.GATES):
            tag = (n, layout, gate)
            stride = n + 5 * (j & 1)
            data = g.columns(100 * n + j, n, gate.n_vec, layout, stride, edge=layout == g.CANON_LE and j % 2 == 0)
            terms = gate.lib_terms(msm_pkg, layout)
            got = msm_pkg.host_fr_gate_eval(data, terms, n, gate.n_vec, stride, gate.rot_step, scalar_layout=layout, threads=3,
                                            out=POISON * n)
            assert got == g.evaluate(data, layout, gate, n, stride), tag
            assert msm_pkg.fr_gate_check(terms, gate.n_vec, n, gate.rot_step) == (gate.degree, len(gate.offsets(n))), tag


def test_column_255_of_256(msm_pkg):
    n, layout = 4, g.MONT_LE
    gate = g.Gate("last-column", 256, [(1, [(255, 1), 0]), (R - 1, [(255, -1)])])
    data = g.columns(255, n, 256, layout, n + 5)
    assert msm_pkg.host_fr_gate_eval(data, gate.lib_terms(msm_pkg, layout), n, 256, n + 5) == g.evaluate(data, layout, gate, n, n + 5)


@pytest.mark.parametrize("n,period", [(256, 1), (256, 4), (256, 256), (1024, 1), (1024, 4), (1024, 256), (1000, 8)])
def test_accumulate_and_scale(msm_pkg, n, period):
    for layout in g.LAYOUTS:
        gate = g.NEIGHBOURS
        terms = gate.lib_terms(msm_pkg, layout)
        data = g.columns(n + period, n, gate.n_vec, layout)
        old, k_acc, scale = g.records(1, n, layout), g.records(2, 1, layout), g.records(3, period, layout)
        twin = lambda **kw: msm_pkg.host_fr_gate_eval(data, terms, n, gate.n_vec, scalar_layout=layout, threads=2, **kw)  # noqa: E731
        assert twin(scale=scale) == g.evaluate(data, layout, gate, n, scale=scale)
        assert twin(flags=g.ACCUMULATE, k_acc=k_acc, out=old) == g.evaluate(data, layout, gate, n, old=old, k_acc=k_acc)
        assert twin(flags=g.ACCUMULATE, k_acc=k_acc, out=old, scale=scale) == \
            g.evaluate(data, layout, gate, n, old=old, k_acc=k_acc, scale=scale)


def test_accumulate_chain_is_one_evaluation(msm_pkg):
    """three gates folded by y as halo2 folds them: ((g0) y + g1) y + g2, against one big-integer evaluation"""
    n, layout = 257, g.MONT_LE
    gates = (g.NEIGHBOURS, g.Gate("b", 2, [(3, [(1, 2), 1])]), g.Gate("c", 2, [(R - 1, [0]), (1, [(1, -1)])]))
    data = g.columns(77, n, 2, layout)
    y = g.records(5, 1, layout)
    out = POISON * n
    for k, gate in enumerate(gates):
        out = msm_pkg.host_fr_gate_eval(data, gate.lib_terms(msm_pkg, layout), n, 2, flags=g.ACCUMULATE if k else 0, k_acc=y, out=out)
    cols, yy = m.tables(data, layout, n, 2), m.decode(y, layout)[0]
    v = [g.rows_ints(cols, gate, gate.coeff_values(layout)) for gate in gates]
    assert out == m.encode([((a * yy + b) * yy + c) % R for a, b, c in zip(*v)], layout)


def test_thread_counts_give_the_same_bytes(msm_pkg):
    n, layout, gate = 5000, g.MONT_LE, g.EIGHT_OFFSETS
    data = g.columns(9, n, gate.n_vec, layout)
    terms = gate.lib_terms(msm_pkg, layout)
    one, many = (msm_pkg.host_fr_gate_eval(data, terms, n, gate.n_vec, threads=k) for k in (1, 16))
    assert one == many == g.evaluate(data, layout, gate, n)


def test_empty_calls_touch_nothing(msm_pkg):
    terms = g.COPY.lib_terms(msm_pkg, g.MONT_LE)
    assert msm_pkg.host_fr_gate_eval(b"", terms, 0, 1) == b""
    assert msm_pkg.host_fr_gate_eval(b"", None, 4, 0, out=POISON * 4) == POISON * 4


def test_every_refusal_of_the_check_by_text(msm_pkg):
    cases = g.check_errors(msm_pkg)
    assert len({text for *_, text in cases.values()}) == 9
    for name, (terms, n_vec, n, rot_step, text) in cases.items():
        with pytest.raises(msm_pkg.MsmError) as e:
            msm_pkg.fr_gate_check(terms, n_vec, n, rot_step)
        assert e.value.status == msm_pkg.INPUT_ERROR and msm_pkg.fr_gate_last_error() == text, name
        if n and n_vec and not n >> 32:   # the twin shares the check (an empty call passes before it looks at the list)
            with pytest.raises(msm_pkg.MsmError):
                msm_pkg.host_fr_gate_eval(b"\0" * 64 * 16, terms, n, n_vec, rot_step=rot_step)
            assert msm_pkg.fr_gate_last_error() == text, name
    good = g.Gate("good", 2, [(1, [0, (1, 1)])]).lib_terms(msm_pkg, g.MONT_LE)
    assert msm_pkg.fr_gate_check(good, 2, 16) == (2, 2) and msm_pkg.fr_gate_last_error() == ""
    # eight offsets pass where nine do not; at n = 8 the nine rotations 0 .. 8 are eight offsets
    nine = cases["nine offsets"][0]
    assert msm_pkg.fr_gate_check(nine, 2, 8) == (5, 8)


def test_every_refusal_of_the_call_by_text(msm_pkg):
    n, layout = 16, g.MONT_LE
    gate = g.NEIGHBOURS
    terms = gate.lib_terms(msm_pkg, layout)
    data = g.columns(1, n, 2, layout)
    rec = g.records(1, 8, layout)
    lib = msm_pkg.lib()

    def refused(text, *, layout=layout, flags=0, data=data, n=n, n_vec=2, stride=n, k_acc=None, scale=None, period=0, out=True):
        buf = ctypes.create_string_buffer(POISON * 16, 32 * 16) if out is True else out
        st = lib.msm_amd_host_fr_gate_eval(layout, flags, msm_pkg._terms_ptr(terms), data, n, n_vec, stride, 1, k_acc, scale, period, 1, buf)
        assert st == msm_pkg.INPUT_ERROR and msm_pkg.fr_gate_last_error() == text, text
        if out is True:
            assert buf.raw == POISON * 16, text

    scalars = "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only"
    refused(scalars, layout=msm_pkg.SCALAR_CANON_BE32)
    refused(scalars, layout=7)
    refused("flags must be 0 or MSM_AMD_GATE_ACCUMULATE", flags=2)
    refused("n >= 2^32", n=1 << 32)
    refused("stride < n", stride=n - 1)
    refused("n_vec * stride >= 2^32", stride=1 << 31)
    refused("null pointer with work to do", data=None)
    refused("null pointer with work to do", out=None)
    refused("null k_acc32 with MSM_AMD_GATE_ACCUMULATE", flags=g.ACCUMULATE)
    period = "period must be a power of two, 1 .. 256, that divides n"
    for bad in (0, 3, 32, 512):   # 32 does not divide 16
        refused(period, scale=rec * 64, period=bad)
    both = ctypes.create_string_buffer(data, len(data) + 32 * n)
    at = ctypes.addressof(both)
    overlap = "the output must be disjoint from all of the input"
    for shift in (0, 32 * (2 * n - 1)):   # out on the first and on the last input record
        st = lib.msm_amd_host_fr_gate_eval(layout, 0, msm_pkg._terms_ptr(terms), at, n, 2, n, 1, None, None, 0, 1, at + shift)
        assert st == msm_pkg.INPUT_ERROR and msm_pkg.fr_gate_last_error() == overlap and both.raw[:len(data)] == data
    st = lib.msm_amd_host_fr_gate_eval(layout, 0, msm_pkg._terms_ptr(terms), at, n, 2, n, 1, None, None, 0, 1, at + 32 * 2 * n)
    assert st == msm_pkg.OK and both.raw[len(data):] == g.evaluate(data, layout, gate, n)


def test_plan_counts_of_hand_worked_lists(msm_pkg):
    """[launches, workgroups of 256 lanes, records read, products, offsets, ctx bytes, degree]"""
    layout = g.MONT_LE
    keys = ("launches", "workgroups", "reads", "products", "offsets", "bytes", "degree")
    plan = lambda gate, n, **kw: msm_pkg.test_fr_gate_plan(gate.lib_terms(msm_pkg, layout), n, gate.n_vec, gate.rot_step, **kw)  # noqa: E731
    # the vanilla gate: 2 + 2 + 3 + 2 + 1 = 10 factors; products 1 + 1 + 2 + 1 + 0, every coefficient 1 or r - 1
    assert plan(g.VANILLA, 1 << 20) == dict(zip(keys, (1, 4096, 10, 5, 1, 0, 3)))
    # a copy of 257 rows under accumulate and a scale of period 1: one factor and two more records, two products
    assert plan(g.COPY, 257, flags=g.ACCUMULATE, period=1) == dict(zip(keys, (1, 2, 3, 2, 1, 32, 1)))
    # 7 x^8 at one row: seven products and the coefficient's; scale of 1 record
    assert plan(g.POWER, 1, period=1) == dict(zip(keys, (1, 1, 9, 9, 1, 32, 8)))
    # rotations -1, 0, 1 at n = 1000: terms of 2, 1, 2 factors, coefficients 1, r - 1, 5; period 8 -> 256 bytes
    assert plan(g.NEIGHBOURS, 1000, period=8) == dict(zip(keys, (1, 4, 6, 4, 3, 256, 2)))
    for gate in g.GATES:
        p = plan(gate, 1000, flags=g.ACCUMULATE)
        assert (p["reads"], p["products"], p["offsets"], p["degree"]) == \
            (gate.factors + 1, gate.products(layout, accumulate=True), len(gate.offsets(1000)), gate.degree), gate
    with pytest.raises(msm_pkg.MsmError):
        plan(g.COPY, 1000, period=16)
    assert msm_pkg.fr_gate_last_error() == "period must be a power of two, 1 .. 256, that divides n"
