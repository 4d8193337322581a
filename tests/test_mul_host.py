"""Host tests (no GPU) of the batch scalar multiplication: the host twins msm_amd_host_mul_points /
msm_amd_host_g2_mul_points against the big-integer models byte for byte -- both groups, both base modes, every input
layout, both output layouts, the three scalar layouts, the planted scalars and bases, the batched normalisation at its
group edges -- and the argument rules.  No expected value comes from the code under test."""
import ctypes
import os
import random

import pytest

import check_ref as c
import mul_ref as m
import test_g2_host as th

GROUPS = [1, 2]
MODES = [m.EACH, m.ONE]


def host_mul(msm_pkg, group, mode, ks, bases, scalar_layout=0, layout_in=0, layout_out=0, threads=0, z=1):
    """bases: affine points (None = identity); one of them for BASE_ONE"""
    pts = b"".join(m.base_record(group, layout_in, p, z) for p in bases)
    return msm_pkg.host_mul_points(m.scalars_bytes(ks, scalar_layout), pts, len(ks), mode, scalar_layout, layout_in,
                                   layout_out, g2=group == 2, threads=threads)


def want(group, layout_out, ks, bases):
    """bases: one per scalar"""
    return b"".join(m.out_record(group, layout_out, m.expected(group, k, p)) for k, p in zip(ks, bases))


def records(buf, size):
    return [buf[i:i + size] for i in range(0, len(buf), size)]


def assert_same(got, exp, group, layout_out, names=None):
    size = m.OUT_BYTES[(group, layout_out)]
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(records(got, size), records(exp, size))):
        assert a == b, (i, names[i] if names else None)


def test_new_symbols_and_plan(msm_pkg):
    L = msm_pkg.lib()
    for name in ("msm_amd_mul_points", "msm_amd_mul_points_device", "msm_amd_g2_mul_points", "msm_amd_g2_mul_points_device",
                 "msm_amd_host_mul_points", "msm_amd_host_g2_mul_points", "msm_amd_test_mul_plan"):
        assert hasattr(L, name) and name in msm_pkg.EXPORTS
    header = open(os.path.join(th.ROOT, "include", "msm_amd.h")).read()
    assert "MSM_AMD_MUL_BASE_EACH = 0" in header and "MSM_AMD_MUL_BASE_ONE = 1" in header
    assert (msm_pkg.MUL_BASE_EACH, msm_pkg.MUL_BASE_ONE) == (0, 1)
    for group in GROUPS:
        plan = msm_pkg.mul_plan(group)
        assert plan["c"] >= 2 and plan["W"] == 254 // plan["c"] + 1 and plan["entries"] == plan["W"] << (plan["c"] - 1)
        assert plan["K"] >= 2
    out = (ctypes.c_uint32 * 4)()
    assert L.msm_amd_test_mul_plan(0, out) == msm_pkg.INPUT_ERROR and L.msm_amd_test_mul_plan(3, out) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_test_mul_plan(1, None) == msm_pkg.INPUT_ERROR


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_planted_scalars_on_the_generator(msm_pkg, group, mode):
    plan = msm_pkg.mul_plan(group)
    ks, names = m.planted_scalars(plan["c"], plan["W"])
    rng = random.Random(7 + group)
    ks += [rng.randrange(m.R) for _ in range(8)]
    names += ["random"] * 8
    gen = m.GEN[group]
    bases = [gen] * (len(ks) if mode == m.EACH else 1)
    got = host_mul(msm_pkg, group, mode, ks, bases, threads=3)
    assert_same(got, want(group, 0, ks, [gen] * len(ks)), group, 0, names)
    size = m.OUT_BYTES[(group, 0)]
    assert records(got, size)[0] == bytes(size) and records(got, size)[1] == m.out_record(group, 0, gen)   # s = 0, s = 1


@pytest.mark.parametrize("group", GROUPS)
def test_every_layout(msm_pkg, group):
    """every scalar layout x input layout x output layout x base mode on one small case; the canonical scalar layouts
    carry integers above r as well (the library reduces them as the MSM does)"""
    rng = random.Random(40 + group)
    n = 9
    pts = m.random_points(group, n, 3)
    pts[4] = None                                                      # an identity base
    ks = [rng.randrange(m.R) for _ in range(n)]
    ks[2] = 0
    big = [k + m.R * (j % 5) for j, k in enumerate(ks)]               # k + 4 r < 5 r < 2^256
    zs = {c.ARK_PROJECTIVE: 1, c.JAC_BE32: rng.randrange(2, c.P)}
    for sl in m.SCALAR_LAYOUTS:
        scal = ks if sl == 0 else big
        for li in m.IN_LAYOUTS[group]:
            z = zs.get(li, 1) if group == 1 else 1
            for lo in m.OUT_LAYOUTS[group]:
                got = host_mul(msm_pkg, group, m.EACH, scal, pts, sl, li, lo, threads=2, z=z)
                assert_same(got, want(group, lo, ks, pts), group, lo)
                got1 = host_mul(msm_pkg, group, m.ONE, scal, [pts[0]], sl, li, lo, threads=2, z=z)
                assert_same(got1, want(group, lo, ks, [pts[0]] * n), group, lo)


def test_g1_jacobian_bases_with_random_z(msm_pkg):
    rng = random.Random(5)
    n = 6
    pts = m.random_points(1, n, 8)
    ks = [rng.randrange(m.R) for _ in range(n)]
    for li in (c.ARK_PROJECTIVE, c.JAC_BE32):
        recs = b"".join(m.base_record(1, li, p, rng.randrange(2, c.P)) for p in pts)
        got = msm_pkg.host_mul_points(m.scalars_bytes(ks, 0), recs, n, m.EACH, 0, li, 0)
        assert_same(got, want(1, 0, ks, pts), 1, 0)


@pytest.mark.parametrize("group", GROUPS)
def test_identity_bases_of_every_layout(msm_pkg, group):
    ks = [0, 1, 2, m.R - 1, 12345]
    for li in m.IN_LAYOUTS[group]:
        for lo in m.OUT_LAYOUTS[group]:
            ident = m.out_record(group, lo, None) * len(ks)
            assert host_mul(msm_pkg, group, m.EACH, ks, [None] * len(ks), 0, li, lo) == ident
            assert host_mul(msm_pkg, group, m.ONE, ks, [None], 0, li, lo) == ident
    if group == 1:                                                     # Z = 0 with any X, Y is the identity
        rec = c.Rec(1, c.ARK_PROJECTIVE, [5, 7, 0]).encode()
        assert msm_pkg.host_mul_points(m.scalars_bytes([3], 0), rec, 1, m.EACH, 0, c.ARK_PROJECTIVE, 0) == bytes(64)
    else:                                                              # a flagged ark record, garbage coordinates
        rec = c.Rec(2, c.G2_ARK, [c.MAX256] * 4, flag=1).encode()
        assert msm_pkg.host_mul_points(m.scalars_bytes([3], 0), rec, 1, m.ONE, 0, c.G2_ARK, 0, g2=True) == bytes(128)


@pytest.mark.parametrize("mode", MODES)
def test_g2_base_of_order_10069(msm_pkg, mode):
    """partial sums of the ladder meet the base and its negative: the doubling and the vanishing branch of the mixed
    addition are taken; [s] P = O whenever 10069 | s"""
    small = m.small_order_point()
    q = m.ORDER_SMALL
    rng = random.Random(9)
    ks = [q, q - 1, q + 1, 2 * q, 2 * q - 1, 3 * q + 1, q * q, q << 100, (q << 100) + 1, 1, 2, 3, q // 2, q // 2 + 1]
    ks += [q * rng.randrange(1, m.R // q) for _ in range(6)] + [rng.randrange(m.R) for _ in range(12)]
    n = len(ks)
    if mode == m.EACH:
        bases = [small if i % 2 == 0 else m.g.neg(small) for i in range(n)]
        got = host_mul(msm_pkg, 2, mode, ks, bases)
    else:
        bases = [small] * n
        got = host_mul(msm_pkg, 2, mode, ks, [small])
    exp = want(2, 0, ks, bases)
    assert_same(got, exp, 2, 0)
    for i, k in enumerate(ks):
        assert (records(got, 128)[i] == bytes(128)) == (k % q == 0), i
    # the model agrees with itself: [s] P depends on s mod 10069 only
    assert m.expected(2, ks[-1], small) == m.expected(2, ks[-1] % q, small)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_batched_normalisation(msm_pkg, group, mode):
    K = msm_pkg.mul_plan(group)["K"]
    pts = m.random_points(group, 2 * K + 1, 21)
    for n in (1, K - 1, K, K + 1, 2 * K + 1):
        for whole in (False, True):
            ks = m.normalisation_case(K, n, 100 * n + whole, whole)
            bases = pts[:n] if mode == m.EACH else [pts[0]] * n
            lo = m.OUT_LAYOUTS[group][n % 2]
            got = host_mul(msm_pkg, group, mode, ks, bases if mode == m.EACH else bases[:1], layout_out=lo, threads=1 + n % 3)
            assert_same(got, want(group, lo, ks, bases), group, lo)
            ident = m.out_record(group, lo, None)
            size = len(ident)
            assert [i for i in range(n) if records(got, size)[i] == ident] == [i for i in range(n) if ks[i] == 0]
    # nothing but identities
    for n in (1, K, K + 1):
        bases = pts[:n] if mode == m.EACH else pts[:1]
        assert host_mul(msm_pkg, group, mode, [0] * n, bases) == m.out_record(group, 0, None) * n


@pytest.mark.parametrize("group", GROUPS)
def test_one_base_equals_each_on_the_replicated_base(msm_pkg, group):
    rng = random.Random(77)
    n = 40
    base = m.random_points(group, 1, 31)[0]
    ks = [rng.randrange(m.R) for _ in range(n)]
    one = host_mul(msm_pkg, group, m.ONE, ks, [base], threads=1)
    each = host_mul(msm_pkg, group, m.EACH, ks, [base] * n, threads=4)
    assert one == each
    assert_same(one[:3 * m.OUT_BYTES[(group, 0)]], want(group, 0, ks[:3], [base] * 3), group, 0)


# ---- the model at every position -----------------------------------------------------------------------------------------------
def encoded(group, layout_out, points):
    return b"".join(m.out_record(group, layout_out, p) for p in points)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [257, 4099])
def test_scalar_progression_one_base(msm_pkg, group, n):
    """s_i = s_0 + i d on a random base: all n records against additions of the model"""
    ks, base, exp = m.scalar_progression(group, 4099)
    lo = m.OUT_LAYOUTS[group][n % 2]
    got = host_mul(msm_pkg, group, m.ONE, ks[:n], [base], layout_out=lo)
    assert_same(got, encoded(group, lo, exp[:n]), group, lo)


@pytest.mark.parametrize("group", GROUPS)
def test_whole_table_and_digit_edges(msm_pkg, group):
    """every table entry alone, every negated entry with its carry, the digit rule at 0x7f / 0x80 / 0x81 / 0xff"""
    plan = msm_pkg.mul_plan(group)
    ks, names, base, exp = m.table_case(group, plan["c"], plan["W"])
    got = host_mul(msm_pkg, group, m.ONE, ks, [base], scalar_layout=1)
    assert_same(got, encoded(group, 0, exp), group, 0, names)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("which", ["random", "r - 1"])
def test_base_progression_each(msm_pkg, group, which):
    """P_i = P_0 + i Q under one scalar: all n records"""
    s = m.R - 1 if which == "r - 1" else random.Random(808).randrange(m.R)
    bases, exp = m.base_progression(group, s, 257)
    got = host_mul(msm_pkg, group, m.EACH, [s] * 257, bases, scalar_layout=2)
    assert_same(got, encoded(group, 0, exp), group, 0)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_star_scalar_doubles_in_the_last_addition(msm_pkg, group, mode):
    """s* = 96 2^248 - r and its neighbours, s* also stored as s* + r and s* + 4 r: the last mixed addition of the digit
    walk meets its own table entry"""
    stored, ks = m.star_scalars()
    for base, layouts in m.star_bases(group):
        exp = encoded(group, 0, [m.expected(group, k, base) for k in ks])
        for sl in layouts:                                    # the Montgomery layout stores the reduced scalar
            got = host_mul(msm_pkg, group, mode, stored if sl else ks, [base] * (len(ks) if mode == m.EACH else 1),
                           scalar_layout=sl)
            assert_same(got, exp, group, 0)


def order3_case(mode, y):
    ks = m.order3_scalars()
    pt = (0, y % c.P)
    bases = [pt if mode == m.ONE or i % 2 == 0 else m.neg(1, pt) for i in range(len(ks))]
    return ks, bases, [m.expected(1, k, b) for k, b in zip(ks, bases)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("y", m.ORDER3_Y)
def test_g1_base_of_order_3(msm_pkg, mode, y):
    """(0, y) has order 3 under the chord-and-tangent formulas (a = 0, b is never read): every ladder step and every
    digit meets acc == +-P, and the fixed-base table holds identity entries.  This pins the branch behaviour of the
    additions (doubling, vanishing sum, identity entry); it is not an API promise -- the header leaves bases off the
    curve unspecified."""
    ks, bases, exp = order3_case(mode, y)
    got = host_mul(msm_pkg, 1, mode, ks, bases if mode == m.EACH else bases[:1])
    assert_same(got, encoded(1, 0, exp), 1, 0)
    for i, k in enumerate(ks):
        assert (records(got, 64)[i] == bytes(64)) == (k % 3 == 0), i


def test_argument_errors(msm_pkg):
    L, IE, OK = msm_pkg.lib(), msm_pkg.INPUT_ERROR, msm_pkg.OK
    sc, pts, out = ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(136 * 4), ctypes.create_string_buffer(136 * 4)
    cases = [(L.msm_amd_host_mul_points, (0, 1, 2, 3), (msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9, -1), (0, 2),
              (msm_pkg.POINT_ARK_PROJECTIVE, msm_pkg.POINT_JAC_BE32, msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9, -1)),
             (L.msm_amd_host_g2_mul_points, (0, 1), (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, 9, -1), (0, 1),
              (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, 9, -1))]
    for fn, in_ok, in_bad, out_ok, out_bad in cases:
        for mode in MODES:
            for li in in_ok:
                for lo in out_ok:
                    assert fn(1, li, mode, sc, pts, 4, lo, 1, out) == OK
            for li in in_bad:
                assert fn(1, li, mode, sc, pts, 4, out_ok[0], 1, out) == IE
            for lo in out_bad:
                assert fn(1, in_ok[0], mode, sc, pts, 4, lo, 1, out) == IE
        for mode in (2, -1):
            assert fn(1, in_ok[0], mode, sc, pts, 4, out_ok[0], 1, out) == IE
        for sl in (3, -1):
            assert fn(sl, in_ok[0], 0, sc, pts, 4, out_ok[0], 1, out) == IE
        assert fn(1, in_ok[0], 0, None, pts, 4, out_ok[0], 1, out) == IE
        assert fn(1, in_ok[0], 0, sc, None, 4, out_ok[0], 1, out) == IE
        assert fn(1, in_ok[0], 0, sc, pts, 4, out_ok[0], 1, None) == IE
        assert fn(1, in_ok[0], 0, sc, pts, 1 << 32, out_ok[0], 1, out) == IE
        assert fn(1, in_ok[0], 0, None, None, 0, out_ok[0], 1, None) == OK          # n == 0 touches nothing
        assert fn(1, in_bad[0], 0, None, None, 0, out_ok[0], 1, None) == IE         # ... but the layouts are still judged


def mul_kernels_scratch():
    """private segment size per kernel of k_mul.hip's code object, read the way test_g2_host reads k_g2's"""
    return th.kernel_scratch(os.path.join(th.CSRC, "k_mul.o"))


def test_mul_kernels_use_no_scratch():
    kernels = mul_kernels_scratch()
    for stem in ("mul_table_kernel", "mul_fixed_kernel", "mul_each_kernel", "mul_normalise_kernel"):
        ours = {k: v for k, v in kernels.items() if stem in k}
        assert len(ours) == 2, (stem, kernels)                                     # the G1 and the G2 instance
        assert all(v == 0 for v in ours.values()), ours
