"""Host twin of the transform over G1 points (msm_amd_host_ntt_points, msm_amd_test_host_ntt_points_levels) against the
model of ntt_points_ref: every position for log_n = 0 .. 7, both directions, both roots, the layouts crossed; the
planted vectors at every position and every level; the round trip, the Lagrange identity, the refused arguments and the
scratch use of the new kernels.  No GPU."""
import ctypes
import os
import random

import pytest

import check_ref as c
import ntt_points_ref as npr
import ntt_ref
import test_g2_host as th

F, I = npr.FORWARD, npr.INVERSE
LOGS = tuple(range(8))


def records(data, size):
    return [data[i:i + size] for i in range(0, len(data), size)]


def check_positions(got, vals, layout, what):
    size = npr.OUT_BYTES[layout]
    assert len(got) == size * len(vals), what
    for k, (rec, v) in enumerate(zip(records(got, size), vals)):
        assert rec == npr.out_record(v, layout), (what, "position", k)


def test_new_symbols(msm_pkg):
    L = msm_pkg.lib()
    for name in ("msm_amd_ntt_points", "msm_amd_ntt_points_device", "msm_amd_host_ntt_points",
                 "msm_amd_test_ntt_points_levels", "msm_amd_test_host_ntt_points_levels"):
        assert hasattr(L, name) and name in msm_pkg.EXPORTS, name
    for name in ("ntt_points", "ntt_points_device", "test_ntt_points_levels"):
        assert hasattr(msm_pkg.MsmConfig, name), name


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("direction", (F, I))
@pytest.mark.parametrize("root", ntt_ref.ROOTS)
def test_every_position_layouts_crossed(msm_pkg, root, direction, log_n):
    a = list(npr.random_logs(log_n))
    want = npr.transform(a, root, log_n, direction)
    for li in npr.IN_LAYOUTS:
        data = npr.in_records(a, li, seed=li + 1)
        for lo in npr.OUT_LAYOUTS:
            got = msm_pkg.host_ntt_points(data, root, log_n, direction, li, lo, threads=1 + (li + lo) % 4)
            check_positions(got, want, lo, (root, direction, log_n, li, lo))


@pytest.mark.parametrize("log_n", (1, 2, 3, 7))
@pytest.mark.parametrize("direction", (F, I))
def test_planted_vectors_at_every_level(msm_pkg, direction, log_n):
    root = npr.H2C if log_n % 2 else npr.ARK
    for name, a in npr.planted(root, log_n, direction).items():
        data = npr.in_records(a, c.H2C)
        states = list(npr.level_states(a, root, log_n, direction))
        for levels, state in enumerate(states):
            got = msm_pkg.test_host_ntt_points_levels(data, root, log_n, levels, direction, threads=3)
            check_positions(got, state, c.H2C, (name, direction, log_n, "levels", levels))
        want = npr.transform(a, root, log_n, direction)
        if direction == F:
            assert want == states[-1]
        check_positions(msm_pkg.host_ntt_points(data, root, log_n, direction), want, c.H2C, (name, direction, log_n))
        n = 1 << log_n
        if name == "constant":
            assert sum(1 for v in want if v) == 1 and want[0] != 0
        if name == "geometric":
            assert [k for k, v in enumerate(want) if v] == [1 % n]
        if name == "zeros":
            assert want == [0] * n


def test_planted_doubling_is_in_a_laddered_lane():
    for direction in (F, I):
        a = npr.planted(npr.ARK, 5, direction)["doubling"]
        s1 = list(npr.level_states(a, npr.ARK, 5, direction))[1]
        w = ntt_ref.omega(npr.ARK, 5)
        q = pow(pow(w, -1, npr.R) if direction == I else w, 8, npr.R)
        assert q != 1 and s1[1] == q * s1[3] % npr.R and a[0] == q * a[16] % npr.R


@pytest.mark.parametrize("log_n", (0, 1, 4, 6))
def test_inverse_of_forward_is_the_input(msm_pkg, log_n):
    a = list(npr.random_logs(log_n))
    for root in ntt_ref.ROOTS:
        for lo in npr.OUT_LAYOUTS:
            x = npr.out_records(a, lo)
            fwd = msm_pkg.host_ntt_points(x, root, log_n, F, lo, lo)
            assert msm_pkg.host_ntt_points(fwd, root, log_n, I, lo, lo) == x
            inv = msm_pkg.host_ntt_points(x, root, log_n, I, lo, lo)
            assert msm_pkg.host_ntt_points(inv, root, log_n, F, lo, lo) == x


def test_lagrange_identity(msm_pkg):
    log_n, n = 6, 64
    tau = random.Random(2024).randrange(2, npr.R)
    srs = [pow(tau, j, npr.R) for j in range(n)]
    got = msm_pkg.host_ntt_points(npr.in_records(srs, c.H2C), npr.H2C, log_n, I)
    check_positions(got, npr.lagrange_at(tau, npr.H2C, log_n), c.H2C, "lagrange")


def test_threads_do_not_change_a_byte(msm_pkg):
    a = list(npr.random_logs(6))
    data = npr.in_records(a, c.ARK_AFFINE)
    ref = msm_pkg.host_ntt_points(data, npr.H2C, 6, I, c.ARK_AFFINE, c.H2C, threads=1)
    for t in (0, 2, 5, 16, 64):
        assert msm_pkg.host_ntt_points(data, npr.H2C, 6, I, c.ARK_AFFINE, c.H2C, threads=t) == ref


def test_argument_errors(msm_pkg):
    L, IE, OK = msm_pkg.lib(), msm_pkg.INPUT_ERROR, msm_pkg.OK
    fn, lv = L.msm_amd_host_ntt_points, L.msm_amd_test_host_ntt_points_levels
    pts, out = ctypes.create_string_buffer(96 * 4), ctypes.create_string_buffer(96 * 4)
    in_bad = (msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9, -1)
    out_bad = (msm_pkg.POINT_ARK_PROJECTIVE, msm_pkg.POINT_JAC_BE32, msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9, -1)
    for li in npr.IN_LAYOUTS:
        for lo in npr.OUT_LAYOUTS:
            assert fn(0, 2, 0, li, pts, lo, out, 1) == OK
    for li in in_bad:
        assert fn(0, 2, 0, li, pts, 0, out, 1) == IE
        assert lv(0, 2, 0, li, pts, 1, 0, out, 1) == IE
    for lo in out_bad:
        assert fn(0, 2, 0, 0, pts, lo, out, 1) == IE
        assert lv(0, 2, 0, 0, pts, 1, lo, out, 1) == IE
    for root in (2, -1):
        assert fn(root, 2, 0, 0, pts, 0, out, 1) == IE
    for direction in (2, -1):
        assert fn(0, 2, direction, 0, pts, 0, out, 1) == IE
    assert fn(0, 29, 0, 0, pts, 0, out, 1) == IE
    assert fn(0, 2, 0, 0, None, 0, out, 1) == IE
    assert fn(0, 2, 0, 0, pts, 0, None, 1) == IE
    assert lv(0, 2, 0, 0, pts, 3, 0, out, 1) == IE                  # levels > log_n
    assert lv(0, 2, 0, 0, pts, 0xFFFFFFFF, 0, out, 1) == IE
    assert lv(0, 2, 0, 0, pts, 2, 0, out, 1) == OK and lv(0, 2, 0, 0, pts, 0, 0, out, 1) == OK
    with pytest.raises(ValueError):
        msm_pkg.host_ntt_points(bytes(64 * 3), 0, 2)                # not n records


def test_ntt_points_kernels_use_no_scratch():
    kernels = th.kernel_scratch(os.path.join(th.CSRC, "k_nttp.o"))
    for stem in ("nttp_load_kernel", "nttp_level_kernel", "nttp_normalise_kernel", "nttp_scale_kernel"):
        ours = {k: v for k, v in kernels.items() if stem in k}
        assert len(ours) == 1, (stem, kernels)
        assert all(v == 0 for v in ours.values()), ours
