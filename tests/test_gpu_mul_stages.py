"""GPU tests of the stage entry msm_amd_test_mul_stage: mul_fixed_kernel over tables the test wrote and
mul_normalise_kernel on XYZZ records at the edge of the point invariant -- the cases of test_mul_stages_host, with the
exceptional records as the only lane, at lane 63 of a full wave and at lane 0 of the second wave.  Every call asserts
device form == host form byte for byte, and the device bytes against the big-integer models (mul_stage_ref)."""
import ctypes

import pytest

import mul_stage_ref as sr
import test_mul_stages_host as hst

pytestmark = pytest.mark.gpu

GROUPS = [1, 2]


def both(cfg, msm_pkg):
    """a runner for the checks of test_mul_stages_host: the device form, after it was compared with the host form"""
    def run(group, which, layout, data, table, n):
        d = cfg.test_mul_stage(group, which, layout, data, table, n)
        h = msm_pkg.test_mul_stage_host(group, which, layout, data, table, n)
        assert d == h, "device form differs from the host form"
        return d
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_fixed_on_the_model_table(cfg, msm_pkg, group):
    hst.check_fixed_on_the_model_table(both(cfg, msm_pkg), group)


@pytest.mark.parametrize("group", GROUPS)
def test_constructed_tables(cfg, msm_pkg, group):
    assert hst.check_constructed_tables(both(cfg, msm_pkg), group) == 16


@pytest.mark.parametrize("group", GROUPS)
def test_normalise_at_the_invariant(cfg, msm_pkg, group):
    hst.check_normalise(both(cfg, msm_pkg), group)


@pytest.mark.parametrize("group", GROUPS)
def test_normalise_maximal_groups_on_lanes_63_and_64(cfg, msm_pkg, group):
    hst.check_normalise_placement(both(cfg, msm_pkg), group)


def test_argument_errors(cfg, msm_pkg):
    def input_error(*a):
        with pytest.raises(msm_pkg.MsmError) as e:
            cfg.test_mul_stage(*a)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    sc, tb, recs = bytes(32 * 4), bytes(4096 * 128), bytes(288 * 4)
    for group in GROUPS:
        for which in (3, -1):
            input_error(group, which, 0, sc, tb, 4)
        input_error(group, sr.FIXED, 3, sc, tb, 4)
        input_error(group, sr.NORMALISE, 9, recs, None, 4)
        input_error(group, sr.FIXED, 1, None, tb, 4)
        input_error(group, sr.FIXED, 1, sc, None, 4)
        input_error(group, sr.NORMALISE, 0, None, None, 4)
        out = ctypes.create_string_buffer(288 * 4)          # (the wrapper would size its output buffer for 2^32 records)
        assert msm_pkg.lib().msm_amd_test_mul_stage(cfg.h, group, sr.FIXED, 1, sc, tb, 1 << 32, out) == msm_pkg.INPUT_ERROR
        assert msm_pkg.lib().msm_amd_test_mul_stage(cfg.h, group, sr.NORMALISE, 0, recs, None, 1 << 32, out) == msm_pkg.INPUT_ERROR
        assert cfg.test_mul_stage(group, sr.FIXED, 1, None, None, 0) == b""
        # the ctx is as good as before: zero scalars walk to the identity record (ZZ limbs zero)
        raw = cfg.test_mul_stage(group, sr.FIXED, 1, sc, tb, 4)
        assert all(sr.decode_xyzz(group, w) is None for w in sr.unpack_words(raw, group))
    input_error(0, sr.FIXED, 1, sc, tb, 4)
    input_error(3, sr.FIXED, 1, sc, tb, 4)
