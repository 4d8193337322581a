"""The host twins of the multi-point polynomial calls (msm_amd_host_fr_poly_eval_points, msm_amd_host_fr_poly_div_points) and
the plan aid (msm_amd_test_fr_poly_points_plan) against the big-integer model of tests/multiopen_ref.py.  No GPU.  Three
algorithms meet here: the twin divides by X - z_j k times in a row (upstream's div_by_vanishing), the model does schoolbook
long division by the expanded vanishing polynomial, and the identity p = q Z_S + r at a random point goes through neither.
Every comparison is of bytes: the records of a result are unique."""
import ctypes
import random

import pytest

import multiopen_ref as m
import poly_ref as p

R = m.R
SIZES = list(range(1, 71)) + [257, 513]
KS = range(1, m.MAX_POINTS + 1)


def twin_div(msm_pkg, data, z, layout, n_vec, threads, in_place):
    """(quotients, values) through the C entry point, out of place into 0xFF bytes or in place"""
    L, k = msm_pkg.lib(), len(z) // 32
    n = len(data) // 32 // n_vec
    src = ctypes.create_string_buffer(data, len(data))
    out = src if in_place else ctypes.create_string_buffer(b"\xFF" * len(data), len(data))
    vals = ctypes.create_string_buffer(b"\xFF" * (32 * n_vec * k), 32 * n_vec * k)
    assert L.msm_amd_host_fr_poly_div_points(layout, z, k, src, n, n_vec, threads, out, vals) == msm_pkg.OK
    if not in_place:
        assert src.raw == data, "input changed"
    return out.raw, vals.raw


def check_case(msm_pkg, data, z, layout, n_vec, tag):
    k, n = len(z) // 32, len(data) // 32 // n_vec
    exp_q, exp_vals = m.div_points(data, z, layout, n_vec)
    assert exp_vals == m.eval_points(data, z, layout, n_vec), tag
    zero = bytes(32 * min(k, n))
    for v in range(n_vec):                                                  # the top min(k, n) records of every quotient
        assert exp_q[32 * (n * (v + 1) - min(k, n)):32 * n * (v + 1)] == zero, tag
    for threads in (1, 16):
        for in_place in (False, True):
            q, vals = twin_div(msm_pkg, data, z, layout, n_vec, threads, in_place)
            assert m.first_difference(q, exp_q) is None, (tag, threads, in_place)
            assert vals == exp_vals, (tag, threads, in_place)
        assert msm_pkg.host_fr_poly_eval_points(data, z, layout, n_vec, threads) == exp_vals, (tag, threads)


# ---- 1. the twins against the model -----------------------------------------------------------------------------------------
def test_omega_has_order_2_to_20():
    assert pow(m.OMEGA_20, 1 << 20, R) == 1 and pow(m.OMEGA_20, 1 << 19, R) == R - 1


@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("n_vec", [1, 3])
def test_every_size_and_k(msm_pkg, layout, n_vec):
    """every n, every k (n < k included); the kind of point set cycles, and every kind meets the sizes around a word, a
    thread range and a vector boundary"""
    for n in SIZES:
        data = m.encode(m.random_values(17 * n + n_vec, n * n_vec), layout)
        for k in KS:
            sets = m.point_sets(layout, k, n)
            chosen = sets if n in (1, 7, 8, 9, 64, 65, 513) else (sets[(n + k) % 4],)
            for name, z in chosen:
                check_case(msm_pkg, data, z, layout, n_vec, (n, k, name))


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_unreduced_coefficients(msm_pkg, layout):
    for n in (1, 5, 70, 257):
        data = m.raw([((3 * i + 1) * R // 7 + i) % (1 << 256) for i in range(n)])   # 256-bit words on both sides of r
        for k in (1, 2, 3, 8):
            check_case(msm_pkg, data, m.point_sets(layout, k, n)[0][1], layout, 1, (n, k))


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_one_point_is_the_single_point_call(msm_pkg, layout):
    for n in (1, 2, 64, 70, 513):
        data = m.encode(m.random_values(n, 3 * n), layout)
        for name, z in p.special_points(layout):
            q, rem = msm_pkg.host_fr_poly_div_linear(data, z, layout, 3)
            assert msm_pkg.host_fr_poly_div_points(data, z, layout, 3) == (q, rem), (n, name)
            assert msm_pkg.host_fr_poly_eval_points(data, z, layout, 3) == msm_pkg.host_fr_poly_eval(data, z, layout, 3) == rem


def test_threads_change_nothing(msm_pkg):
    layout = m.CANON_LE
    for n, n_vec, k in ((1, 40, 3), (3, 11, 8), (37, 3, 5), (1000, 2, 4)):
        data = m.encode(m.random_values(n, n * n_vec), layout)
        z = m.point_sets(layout, k, n)[3][1]
        base = (msm_pkg.host_fr_poly_div_points(data, z, layout, n_vec, 1), msm_pkg.host_fr_poly_eval_points(data, z, layout, n_vec, 1))
        assert base[0] == m.div_points(data, z, layout, n_vec) and base[1] == base[0][1]
        for threads in (2, 3, 7, 16):
            assert (msm_pkg.host_fr_poly_div_points(data, z, layout, n_vec, threads),
                    msm_pkg.host_fr_poly_eval_points(data, z, layout, n_vec, threads)) == base, (n, threads)


# ---- 2. identities that do not go through the model's division ------------------------------------------------------------
def test_quotient_times_vanishing_plus_remainder(msm_pkg):
    """p(tau) = q(tau) Z_S(tau) + r(tau) at a random tau, r interpolated from the returned values"""
    rng = random.Random(8)
    for layout in m.LAYOUTS:
        for n in (1, 2, 3, 9, 70, 257):
            data = m.encode(m.random_values(3 * n, 2 * n), layout)
            for k in KS:
                for name, z in m.point_sets(layout, k, n + 1):
                    zs = m.point_values(z, layout)
                    q, vals = msm_pkg.host_fr_poly_div_points(data, z, layout, 2)
                    tau = rng.randrange(R)
                    for v, coeffs in enumerate(p.vectors(data, layout, 2)):
                        qi = m.decode(q[32 * n * v:32 * n * (v + 1)], layout)
                        ys = m.decode(vals[32 * k * v:32 * k * (v + 1)], layout)
                        assert ys == [p.eval_ints(coeffs, zj) for zj in zs], (n, k, name)
                        lhs = p.eval_ints(coeffs, tau)
                        assert lhs == (p.eval_ints(qi, tau) * m.vanishing_eval(zs, tau) + m.interpolate_eval(zs, ys, tau)) % R, (n, k, name)


def test_the_identity_of_the_device_on_model_integers():
    """q_i = sum_j w_j s^(j)_(i+1) is the floor quotient, n < k included, and the top records are exact zeros"""
    rng = random.Random(3)
    for n in (1, 2, 3, 4, 5, 9, 70):
        c = [rng.randrange(R) for _ in range(n)]
        for k in KS:
            zs = [rng.randrange(R) for _ in range(k)]            # distinct but for a chance of 2^-250
            w = [pow(m.vanishing_eval([zm for t, zm in enumerate(zs) if t != j], zj), -1, R) for j, zj in enumerate(zs)]
            s = [p.div_linear_horner(c, zj)[0] for zj in zs]                      # s^(j)_(i+1), i < n
            q = [sum(wj * sj[i] for wj, sj in zip(w, s)) % R for i in range(n)]
            assert q == m.div_points_ints(c, zs)[0], (n, k)
            if k > 1:
                assert sum(w) % R == 0
                assert q == [sum(w[j] * (s[j][i] - s[k - 1][i]) for j in range(k - 1)) % R for i in range(n)]


def test_a_repeated_point_repeats_its_value(msm_pkg):
    for layout in m.LAYOUTS:
        n = 70
        data = m.encode(m.random_values(5, 2 * n), layout)
        a, b = m.encode([12345], layout), m.raw([R + 1])
        z = a + b + a + m.raw([1]) + a
        y = msm_pkg.host_fr_poly_eval_points(data, z, layout, 2)
        assert y == m.eval_points(data, z, layout, 2)
        for v in range(2):
            rec = [y[32 * (5 * v + j):32 * (5 * v + j + 1)] for j in range(5)]
            assert rec[0] == rec[2] == rec[4] and rec[1] == rec[3]


# ---- 3. arguments ----------------------------------------------------------------------------------------------------------------
def test_input_errors_leave_the_outputs(msm_pkg):
    L, n, k = msm_pkg.lib(), 8, 3
    a = m.encode(m.random_values(1, 3 * n), m.MONT_LE)
    z = m.encode([5, 6, 7], m.MONT_LE)
    z9 = m.encode(list(range(2, 11)), m.MONT_LE)
    big = ctypes.create_string_buffer(a + a, 2 * len(a))
    base = ctypes.addressof(big)
    out = ctypes.create_string_buffer(b"\xFF" * len(a), len(a))
    y = ctypes.create_string_buffer(b"\xFF" * (32 * 3 * 9), 32 * 3 * 9)
    vp = ctypes.c_void_p
    bad, ok = msm_pkg.INPUT_ERROR, msm_pkg.OK
    fev, fdiv = L.msm_amd_host_fr_poly_eval_points, L.msm_amd_host_fr_poly_div_points
    for layout in (msm_pkg.SCALAR_CANON_BE32, 3, -1):
        assert fev(layout, z, k, a, n, 3, 0, y) == bad
        assert fdiv(layout, z, k, a, n, 3, 0, out, y) == bad
    assert fev(0, z9, 0, a, n, 3, 0, y) == bad and fdiv(0, z9, 0, a, n, 3, 0, out, y) == bad          # k == 0
    assert fev(0, z9, 9, a, n, 3, 0, y) == bad and fdiv(0, z9, 9, a, n, 3, 0, out, y) == bad          # k > 8
    assert fev(0, None, k, a, n, 3, 0, y) == bad and fdiv(0, None, k, a, n, 3, 0, out, y) == bad      # null z
    assert fev(0, None, k, None, 0, 3, 0, y) == bad                                                   # ... in an empty call too
    assert fev(0, z, k, None, n, 3, 0, y) == bad and fev(0, z, k, a, n, 3, 0, None) == bad            # null pointers
    assert fdiv(0, z, k, None, n, 3, 0, out, y) == bad and fdiv(0, z, k, a, n, 3, 0, None, y) == bad
    assert fev(0, z, k, a, 1 << 16, 1 << 16, 0, y) == bad and fdiv(0, z, k, a, 1 << 32, 1, 0, out, y) == bad
    assert fdiv(0, z, k, vp(base), n, 3, 0, vp(base + 32), y) == bad                                  # partial overlap
    assert fdiv(0, z, k, vp(base + 32), n, 3, 0, vp(base), y) == bad
    for layout in m.LAYOUTS:                                                                          # equal mod r
        same = m.raw([1]) + m.encode([9], layout) + m.raw([R + 1])                                    # the words 1 and r + 1
        assert fdiv(layout, same, 3, a, n, 3, 0, out, y) == bad
        assert fdiv(layout, same, 3, vp(base), n, 3, 0, vp(base), y) == bad
        assert fev(layout, same, 3, a, n, 3, 0, y) == ok                                              # the evaluation takes them
        assert y.raw[:32 * 9] == m.eval_points(a, same, layout, 3)
        y = ctypes.create_string_buffer(b"\xFF" * (32 * 3 * 9), 32 * 3 * 9)
    assert out.raw == b"\xFF" * len(a) and y.raw == b"\xFF" * (32 * 3 * 9) and big.raw == a + a
    # nothing to do: OK, nothing touched
    for nn, nv in ((0, 3), (3, 0), (0, 0)):
        assert fev(0, z, k, None, nn, nv, 0, y) == ok and fdiv(0, z, k, None, nn, nv, 0, out, y) == ok
    assert out.raw == b"\xFF" * len(a) and y.raw == b"\xFF" * (32 * 3 * 9)
    assert msm_pkg.host_fr_poly_eval_points(b"", z) == b"" and msm_pkg.host_fr_poly_div_points(b"", z) == (b"", b"")
    assert fdiv(0, z, k, a, n, 3, 0, out, None) == ok and out.raw == m.div_points(a, z, m.MONT_LE, 3)[0]    # vals_out is optional


def test_header_and_exports(msm_pkg):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msm_amd.h")).read()
    for name in ("msm_amd_fr_poly_eval_points", "msm_amd_fr_poly_div_points", "msm_amd_host_fr_poly_eval_points",
                 "msm_amd_host_fr_poly_div_points", "msm_amd_test_fr_poly_points_plan"):
        assert name in msm_pkg.EXPORTS and hasattr(msm_pkg.lib(), name) and name + "(" in header
    assert "MSM_AMD_POLY_MAX_POINTS = 8" in header


# ---- 4. the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, tile_log", [(70, 2), (513, 2), (513, 3), ((1 << 18) + 1, 9)])
def test_plan(msm_pkg, n, tile_log):
    single = msm_pkg.test_fr_plan(n, 2, tile_log)
    for divide in (True, False):
        one, eight = (msm_pkg.test_fr_poly_points_plan(n, 2, k, tile_log, divide) for k in (1, 8))
        assert one["launches"] == eight["launches"] == (single["launches"] if divide else single["levels"])
        assert one["levels"] == eight["levels"] == single["levels"]
        assert one["records"] == single["records"] + 2 and one["bytes"] == 32 * one["records"]      # the single-point call's
        assert eight["records"] == 8 * one["records"] and eight["bytes"] == 32 * eight["records"]
        assert one["arg_bytes"] == eight["arg_bytes"] < 4096
        assert one["level0_waves"] == eight["level0_waves"] == single["tiles"] * (2 if divide and single["levels"] > 1 else 1)
        assert eight["waves"] - eight["level0_waves"] == 8 * (one["waves"] - one["level0_waves"])
    with pytest.raises(msm_pkg.MsmError):
        msm_pkg.test_fr_poly_points_plan(n, 2, 9, tile_log)
    with pytest.raises(msm_pkg.MsmError):
        msm_pkg.test_fr_poly_points_plan(n, 2, 0, tile_log)
