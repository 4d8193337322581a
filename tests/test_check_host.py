"""Host tests of the point validation (no GPU): the host twins msm_amd_host_check_points / msm_amd_host_g2_check_points
-- the bodies the kernels of k_check.hip run, compiled for the CPU -- against the big-integer rule of check_ref for every
layout, every check mask and every planted case; the report arithmetic; argument errors; the constants of the
subgroup test; and the register budget of the kernels (no scratch)."""
import os
import re

import pytest

import check_ref as c
import g2_ref as g
import test_g2_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc")
MASKS = (1, 2, 3)


def run(msm_pkg, group, layout, recs, checks, **kw):
    fn = msm_pkg.host_check_points if group == 1 else msm_pkg.host_g2_check_points
    return fn(c.encode_all(recs), len(recs), checks=checks, point_layout=layout, **kw)


def check_against_model(msm_pkg, group, layout, recs, names, checks):
    want, want_reasons = c.expected_report(recs, checks)
    rep, reasons = run(msm_pkg, group, layout, recs, checks)
    diff = [(i, names[i], reasons[i], want_reasons[i]) for i in range(len(recs)) if reasons[i] != want_reasons[i]]
    assert not diff, diff
    assert c.same_report(rep, want), (rep, want)
    assert sum(rep["by_reason"]) == len(recs) and rep["device_ms"] == 0.0


# ---- 1. every layout, every mask, every planted case -----------------------------------------------------------------
@pytest.mark.parametrize("layout", [c.H2C, c.ARK_PROJECTIVE, c.ARK_AFFINE, c.JAC_BE32])
def test_g1_planted_cases(msm_pkg, layout):
    recs, names = c.g1_case_records(layout, 100 + layout)
    exp = c.expected_reasons(recs, 1)
    assert {c.VALID, c.NOT_REDUCED, c.NOT_ON_CURVE} == set(exp)            # the corpus reaches every G1 reason
    assert exp[names.index("y + 1")] == c.NOT_ON_CURVE and exp[names.index("identity")] == c.VALID
    for checks in MASKS:                                                   # SUBGROUP equals CURVE on G1
        check_against_model(msm_pkg, 1, layout, recs, names, checks)
        assert c.expected_reasons(recs, checks) == exp


@pytest.mark.parametrize("layout", [c.G2_H2C, c.G2_ARK])
def test_g2_planted_cases(msm_pkg, layout):
    recs, names = c.g2_case_records(layout, 200 + layout)
    full = c.expected_reasons(recs, 3)
    assert set(full) == {0, 1, 2, 3}
    for name in ("curve point outside G2", "cofactor point", "G2 point + cofactor point", "point of order 10069"):
        assert full[names.index(name)] == c.NOT_IN_SUBGROUP, name
    assert c.expected_reasons(recs, 2) == full                              # SUBGROUP implies CURVE
    curve_only = c.expected_reasons(recs, 1)
    assert curve_only == bytes(0 if r == 3 else r for r in full)
    for checks in MASKS:
        check_against_model(msm_pkg, 2, layout, recs, names, checks)


def test_g2_subgroup_rule_on_more_points(msm_pkg):
    """[r] P = O is the meaning: random curve points, their cofactor and G2 parts and sums of the two, all on the curve"""
    import random
    rng = random.Random(77)
    pts = []
    for i in range(3):
        q = c.rand_curve_point_g2(rng)
        pts += [q, g.scalar_mul(c.R_ORDER, q), g.scalar_mul(c.COFACTOR, q), g.add(g.scalar_mul(c.COFACTOR, q), q),
                g.scalar_mul(c.X0, q), g.neg(g.scalar_mul(c.COFACTOR * (i + 2), q))]
    pts += [g.scalar_mul(k, g.GEN2) for k in (1, 2, c.X0, c.X0 + 1, 2 * c.X0, 6 * c.X0 * c.X0, c.R_ORDER - 1)]
    recs = [c.g2_rec(c.G2_H2C, p) for p in pts]
    exp = c.expected_reasons(recs, 3)
    assert exp.count(c.VALID) >= 13 and exp.count(c.NOT_IN_SUBGROUP) >= 6
    check_against_model(msm_pkg, 2, c.G2_H2C, recs, [str(i) for i in range(len(recs))], 3)


# ---- 2. the report ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_first_invalid_is_the_smallest_index(msm_pkg, group):
    n = 130
    good = ([c.g1_rec(c.H2C, p) for p in c.g1_points(n, 5)] if group == 1 else
            [c.g2_rec(c.G2_H2C, p) for p in c.g2_points(n, 5)])
    recs = list(good)
    rep, reasons = run(msm_pkg, group, 0, recs, 3)
    assert rep["n_invalid"] == 0 and rep["first_invalid"] is None and rep["first_reason"] == 0
    assert rep["by_reason"] == [n, 0, 0, 0] and reasons == bytes(n) and rep["n_identity"] == 0
    planted = {n - 1: c.non_reduced(good[n - 1], 0),
               64: good[64].with_coord(1, (good[64].coords[1] + 1) % c.P),
               63: good[63].with_coord(0, (good[63].coords[0] + 1) % c.P)}
    for i in (n - 1, 64, 63):                   # inserted in this order: the answer must not depend on it
        recs[i] = planted[i]
    want, want_reasons = c.expected_report(recs, 3)
    assert want["first_invalid"] == 63 and want["n_invalid"] == 3
    for threads in (1, 3, 0):                   # index ranges per thread: 63 and 64 fall into different ranges at 3
        rep, reasons = run(msm_pkg, group, 0, recs, 3, threads=threads)
        assert reasons == want_reasons and c.same_report(rep, want), (threads, rep)
    rep, reasons = run(msm_pkg, group, 0, recs, 3, reasons=False)          # reasons == NULL is accepted
    assert reasons is None and c.same_report(rep, want)


def test_identities_are_counted(msm_pkg):
    recs = [c.g2_rec(c.G2_ARK, None), c.g2_rec(c.G2_ARK, g.GEN2), c.g2_rec(c.G2_ARK, None)]
    rep, reasons = run(msm_pkg, 2, c.G2_ARK, recs, 3)
    assert rep["n_identity"] == 2 and reasons == bytes(3)
    recs = [c.g1_rec(c.JAC_BE32, None), c.Rec(1, c.JAC_BE32, [c.P, 1, 0])]   # Z = 0 but X = p: not reduced, no identity
    rep, reasons = run(msm_pkg, 1, c.JAC_BE32, recs, 1)
    assert rep["n_identity"] == 1 and reasons == bytes([0, 1]) and rep["first_invalid"] == 1


# ---- 3. arguments ----------------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    g1 = c.encode_all([c.g1_rec(c.H2C, p) for p in c.g1_points(2, 1)])
    g2 = c.encode_all([c.g2_rec(c.G2_H2C, p) for p in c.g2_points(2, 1)])

    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR

    for checks in (0, 4, 7, 1 << 31):
        input_error(msm_pkg.host_check_points, g1, 2, checks=checks)
        input_error(msm_pkg.host_g2_check_points, g2, 2, checks=checks)
    for layout in (msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 6, -1):
        input_error(msm_pkg.host_check_points, g1, 2, point_layout=layout)
    for layout in (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, 4, -1):
        input_error(msm_pkg.host_g2_check_points, g2, 2, point_layout=layout)
    input_error(msm_pkg.host_check_points, None, 2)
    input_error(msm_pkg.host_g2_check_points, None, 2)
    input_error(msm_pkg.host_check_points, g1, 1 << 32)
    L = msm_pkg.lib()
    assert L.msm_amd_host_check_points(0, g1, 2, 1, 0, None, None) == msm_pkg.INPUT_ERROR      # no report
    for fn in (msm_pkg.host_check_points, msm_pkg.host_g2_check_points):                      # n == 0: an empty report
        rep, reasons = fn(None, 0)
        assert reasons == b"" and rep["first_invalid"] is None
        assert {k: rep[k] for k in ("n_checked", "n_invalid", "n_identity", "by_reason")} == \
            {"n_checked": 0, "n_invalid": 0, "n_identity": 0, "by_reason": [0, 0, 0, 0]}


def test_constants_of_the_python_binding(msm_pkg):
    assert (msm_pkg.POINT_VALID, msm_pkg.POINT_NOT_REDUCED, msm_pkg.POINT_NOT_ON_CURVE,
            msm_pkg.POINT_NOT_IN_SUBGROUP) == (0, 1, 2, 3)
    assert (msm_pkg.CHECK_CURVE, msm_pkg.CHECK_SUBGROUP) == (1, 2)
    header = open(os.path.join(ROOT, "include", "msm_amd.h")).read()
    for name, value in (("MSM_AMD_POINT_NOT_IN_SUBGROUP", 3), ("MSM_AMD_CHECK_SUBGROUP", 2), ("MSM_AMD_CHECK_CURVE", 1)):
        assert re.search(rf"{name} = {value}\b", header), name


# ---- 4. the constants of check_points.hip.h ----------------------------------------------------------------------------
def _header_constants():
    src = open(os.path.join(CSRC, "check_points.hip.h")).read()
    body = src[src.index("constexpr uint32_t c[6][9]"):]
    body = body[:body.index("};")]
    rows = re.findall(r"\{([^{}]*)\}", body)
    assert len(rows) == 6
    vals = [g.value([int(w.strip().rstrip("u"), 16) for w in row.split(",") if w.strip()]) for row in rows]
    return [(vals[2 * i], vals[2 * i + 1]) for i in range(3)]


def test_twist_constant_and_psi_constants_are_pinned():
    """b' = 3 / (9 + u) against g2_ref.B_TWIST, gx, gy against xi^((p-1)/3), xi^((p-1)/2): internal domain rho = 2^261"""
    b, gx, gy = _header_constants()
    to_internal = lambda a: (a[0] * g.RHO % g.P, a[1] * g.RHO % g.P)
    assert b == to_internal(g.B_TWIST)
    assert g.mul2(g.B_TWIST, (9, 1)) == (3, 0)
    assert gx == to_internal(c.PSI_X) and gy == to_internal(c.PSI_Y)
    src = open(os.path.join(CSRC, "check_points.hip.h")).read()
    three = re.search(r"check_b_g1\(\).*?c\[9\] = \{(.*?)\};", src, re.S).group(1)
    assert g.value([int(w.strip().rstrip("u"), 16) for w in three.split(",") if w.strip()]) == 3 * g.RHO % g.P
    assert f"kBnX0 = {c.X0}ull" in src


def test_endomorphism_identity_in_the_model():
    """the shortcut the kernel evaluates, [x0 + 1] P + psi([x0] P) + psi^2([x0] P) == psi^3([2 x0] P), agrees with
    [r] P == O on the named points (big integers only)"""
    conj = lambda a: (a[0], -a[1] % c.P)
    psi = lambda pt: None if pt is None else (g.mul2(conj(pt[0]), c.PSI_X), g.mul2(conj(pt[1]), c.PSI_Y))
    sp = c.special_g2()
    pts = list(sp.values()) + [g.GEN2, g.scalar_mul(31337, g.GEN2), g.scalar_mul(c.COFACTOR, sp["curve"])]
    for pt in pts:
        assert g.on_curve(psi(pt))
        q = g.scalar_mul(c.X0, pt)
        lhs = g.add(g.add(g.add(q, pt), psi(q)), psi(psi(q)))
        assert (lhs == psi(psi(psi(g.add(q, q))))) == (g.scalar_mul(c.R_ORDER, pt) is None)


# ---- 5. registers ------------------------------------------------------------------------------------------------------
def test_check_kernels_use_no_scratch():
    kernels = th.kernel_scratch(os.path.join(CSRC, "k_check.o"))
    check = {k: v for k, v in kernels.items() if "check_" in k}
    assert any("check_g1_kernel" in k for k in check) and any("check_g2_kernel" in k for k in check), kernels
    assert len(kernels) >= 3 and all(v == 0 for v in kernels.values()), kernels
