"""GPU tests of the point validation: check_g1_kernel / check_g2_kernel against their host twins byte for byte and
against the big-integer rule of check_ref at the planted records, over lane tails, wave boundaries and several
workgroups; the report fields; the host-buffer and the device entry points; argument errors; MSM results of the same
ctx unchanged; the bounded wait."""
import functools

import numpy as np
import pytest

import check_ref as c
import g2_ref as g
import test_g2_host as th

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
MONT_ONE = c.o.fq_to_mont(1).to_bytes(32, "little")


def on_device(cfg, data):
    d = cfg.alloc(len(data))
    cfg.to_device(d, data)
    return d


def drop_ms(rep):
    return {k: v for k, v in rep.items() if k != "device_ms"}


# ---- inputs: valid points from the library's generators (computed once per size), bad ones from check_ref -------------
@functools.lru_cache(maxsize=None)
def valid_g1(msm_pkg, n):
    return msm_pkg.generate_instance_host(c.o.SEED_BASE + 77, n)[0]


@functools.lru_cache(maxsize=None)
def valid_g2(msm_pkg, n):
    return msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(90001, g.GEN2)), g.encode_h2c(g.scalar_mul(7919, g.GEN2)), n)


def g1_in_layout(h2c: bytes, layout):
    """the 64-byte halo2curves records re-encoded: ark projective (Z = 1), ark affine (no flag), wire (BE32 words)"""
    n = len(h2c) // 64
    xy = np.frombuffer(h2c, dtype="<u4").reshape(n, 2, 8)
    if layout == c.H2C:
        return h2c
    if layout == c.ARK_AFFINE:
        return np.concatenate([xy.reshape(n, 16), np.zeros((n, 2), dtype="<u4")], axis=1).tobytes()
    one = np.broadcast_to(np.frombuffer(MONT_ONE, dtype="<u4"), (n, 1, 8))
    xyz = np.concatenate([xy, one], axis=1)
    if layout == c.JAC_BE32:
        xyz = xyz[:, :, ::-1]
    return np.ascontiguousarray(xyz).tobytes()


def bad_g1(layout, seed):
    recs, names = c.g1_case_records(layout, seed)
    exp = c.expected_reasons(recs, 1)
    keep = [i for i in range(len(recs)) if exp[i] or c.is_identity(recs[i])]     # offenders and identity encodings
    return [recs[i] for i in keep]


def bad_g2(layout, seed):
    recs, names = c.g2_case_records(layout, seed)
    exp = c.expected_reasons(recs, 3)
    keep = [i for i in range(len(recs)) if exp[i] or c.is_identity(recs[i])]
    return [recs[i] for i in keep]


def plant(buf: bytes, stride, recs, n, rng):
    """recs at distinct random indices of the n-record array (as many as fit), first and last index included"""
    idx = sorted(rng.sample(range(n), min(n, len(recs))))
    idx[0], idx[-1] = 0, n - 1
    out = bytearray(buf)
    placed = {}
    for i, r in zip(idx, recs):
        out[i * stride:(i + 1) * stride] = r.encode()
        placed[i] = r
    return bytes(out), placed


def check_everywhere(cfg, msm_pkg, group, layout, buf, n, checks, placed):
    """device entry == host-buffer entry == host twin, and all equal the big-integer rule at the planted records"""
    host_fn = msm_pkg.host_check_points if group == 1 else msm_pkg.host_g2_check_points
    buf_fn = cfg.check_points if group == 1 else cfg.g2_check_points
    dev_fn = cfg.check_points_device if group == 1 else cfg.g2_check_points_device
    h_rep, h_reasons = host_fn(buf, n, checks=checks, point_layout=layout)
    b_rep, b_reasons = buf_fn(buf, n, checks=checks, point_layout=layout)
    dp, dr = on_device(cfg, buf), cfg.alloc(n)
    try:
        d_rep = dev_fn(dp, n, checks=checks, point_layout=layout, d_reasons=dr)
        d_reasons = cfg.to_host(dr, n)
        d_rep_null = dev_fn(dp, n, checks=checks, point_layout=layout)           # d_reasons == NULL
    finally:
        cfg.free(dp)
        cfg.free(dr)
    assert d_reasons == h_reasons and b_reasons == h_reasons
    assert drop_ms(d_rep) == drop_ms(h_rep) == drop_ms(b_rep) == drop_ms(d_rep_null), (d_rep, h_rep, b_rep)
    assert d_rep["device_ms"] > 0 and sum(d_rep["by_reason"]) == n == d_rep["n_checked"]
    for i, r in placed.items():
        assert d_reasons[i] == c.expected_reason(r, checks), (i, r.coords)
    bad = [i for i, r in placed.items() if c.expected_reason(r, checks)]
    assert d_rep["n_invalid"] == len(bad) == n - d_reasons.count(0)             # nothing but the planted offenders
    assert d_rep["first_invalid"] == (min(bad) if bad else None)
    assert d_rep["n_identity"] == sum(c.is_identity(r) for r in placed.values())
    return d_rep


# ---- 1. sizes: lane tail, wave boundary, several workgroups ------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_g1_sizes(cfg, msm_pkg, n):
    import random
    rng = random.Random(n)
    layout = (c.H2C, c.ARK_PROJECTIVE, c.ARK_AFFINE, c.JAC_BE32)[SIZES.index(n) % 4]
    buf, placed = plant(g1_in_layout(valid_g1(msm_pkg, n), layout), c.G1_BYTES[layout], bad_g1(layout, n), n, rng)
    check_everywhere(cfg, msm_pkg, 1, layout, buf, n, 1, placed)


@pytest.mark.parametrize("n", SIZES)
def test_g2_sizes(cfg, msm_pkg, n):
    import random
    rng = random.Random(n)
    buf, placed = plant(valid_g2(msm_pkg, n), 128, bad_g2(c.G2_H2C, n), n, rng)
    rep = check_everywhere(cfg, msm_pkg, 2, c.G2_H2C, buf, n, 3, placed)
    if n >= 257:
        assert rep["by_reason"][3] >= 4 and rep["by_reason"][2] >= 3 and rep["by_reason"][1] >= 8
        check_everywhere(cfg, msm_pkg, 2, c.G2_H2C, buf, n, 1, placed)          # CURVE alone: subgroup offenders pass


@pytest.mark.parametrize("layout", [c.H2C, c.ARK_PROJECTIVE, c.ARK_AFFINE, c.JAC_BE32])
def test_g1_every_layout(cfg, msm_pkg, layout):
    import random
    n = 321
    buf, placed = plant(g1_in_layout(valid_g1(msm_pkg, n), layout), c.G1_BYTES[layout], bad_g1(layout, 9), n,
                        random.Random(layout))
    for checks in (1, 2, 3):
        check_everywhere(cfg, msm_pkg, 1, layout, buf, n, checks, placed)


def test_g2_ark_layout(cfg, msm_pkg):
    import random
    n = 130
    h2c = valid_g2(msm_pkg, n)
    ark = b"".join(h2c[128 * i:128 * i + 128] + bytes(8) for i in range(n))
    buf, placed = plant(ark, 136, bad_g2(c.G2_ARK, 4), n, random.Random(4))
    check_everywhere(cfg, msm_pkg, 2, c.G2_ARK, buf, n, 3, placed)


# ---- 2. the report ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_first_invalid_across_workgroups(cfg, msm_pkg, group):
    """Two offenders in different workgroups.  The one with the HIGHER index is rejected at once (a coordinate >= p,
    no arithmetic), the one with the lower index only after the whole check (G2: the subgroup ladder; G1: the curve
    equation), so the higher index reaches the report first: first_invalid must still be the lower one."""
    n = 2048
    if group == 1:
        layout, stride, buf = c.H2C, 64, valid_g1(msm_pkg, n)
        good = c.g1_rec(layout, c.g1_points(1, 3)[0])
        slow = good.with_coord(1, (good.coords[1] + 1) % c.P)
    else:
        layout, stride, buf = c.G2_H2C, 128, valid_g2(msm_pkg, n)
        good = c.g2_rec(layout, g.GEN2)
        slow = c.g2_rec(layout, c.special_g2()["g2_plus_cofactor"])
    fast = c.non_reduced(good, 0, top=True)
    lo, hi = 1000, 1900
    out = bytearray(buf)
    out[hi * stride:(hi + 1) * stride] = fast.encode()
    out[lo * stride:(lo + 1) * stride] = slow.encode()
    rep = check_everywhere(cfg, msm_pkg, group, layout, bytes(out), n, 3, {hi: fast, lo: slow})
    assert rep["first_invalid"] == lo and rep["first_reason"] == (2 if group == 1 else 3)


# ---- 3. one larger grid per group --------------------------------------------------------------------------------------
def test_g1_2p16(cfg, msm_pkg):
    n = 1 << 16
    good = c.g1_rec(c.H2C, c.g1_points(1, 8)[0])
    placed = {n - 1: c.non_reduced(good, 1), 40000: good.with_coord(0, (good.coords[0] + 1) % c.P),
              12345: good.with_coord(1, (good.coords[1] + 1) % c.P), 7: c.g1_rec(c.H2C, None)}
    out = bytearray(valid_g1(msm_pkg, n))
    for i, r in placed.items():
        out[64 * i:64 * i + 64] = r.encode()
    rep = check_everywhere(cfg, msm_pkg, 1, c.H2C, bytes(out), n, 1, placed)
    assert rep["first_invalid"] == 12345 and rep["by_reason"] == [n - 3, 1, 2, 0] and rep["n_identity"] == 1


def test_g2_2p16(cfg, msm_pkg):
    n = 1 << 16
    sp = c.special_g2()
    good = c.g2_rec(c.G2_H2C, g.GEN2)
    placed = {n - 1: c.g2_rec(c.G2_H2C, sp["order_10069"]), 33333: c.non_reduced(good, 3),
              20000: good.with_coord(2, (good.coords[2] + 1) % c.P), 64: c.g2_rec(c.G2_H2C, None)}
    out = bytearray(valid_g2(msm_pkg, n))
    for i, r in placed.items():
        out[128 * i:128 * i + 128] = r.encode()
    rep = check_everywhere(cfg, msm_pkg, 2, c.G2_H2C, bytes(out), n, 3, placed)
    assert rep["first_invalid"] == 20000 and rep["by_reason"] == [n - 3, 1, 1, 1] and rep["n_identity"] == 1


# ---- 4. errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(cfg, msm_pkg):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    n = 64
    g1, g2 = valid_g1(msm_pkg, n), valid_g2(msm_pkg, n)
    d1, d2 = on_device(cfg, g1), on_device(cfg, g2)
    try:
        for layout in (msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9):
            input_error(cfg.check_points, g1, n, point_layout=layout)
            input_error(cfg.check_points_device, d1, n, point_layout=layout)
        for layout in (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, 9):
            input_error(cfg.g2_check_points, g2, n, point_layout=layout)
            input_error(cfg.g2_check_points_device, d2, n, point_layout=layout)
        for checks in (0, 4, 8 | 1):
            input_error(cfg.check_points, g1, n, checks=checks)
            input_error(cfg.g2_check_points_device, d2, n, checks=checks)
        input_error(cfg.check_points, None, n)
        input_error(cfg.g2_check_points_device, None, n)
        input_error(cfg.check_points_device, d1, 1 << 32)
        for rep in (cfg.check_points(None, 0)[0], cfg.check_points_device(None, 0), cfg.g2_check_points(None, 0)[0],
                    cfg.g2_check_points_device(None, 0)):                       # n == 0: OK, an empty report
            assert rep["n_checked"] == 0 and rep["first_invalid"] is None and rep["by_reason"] == [0, 0, 0, 0]
        assert cfg.check_points_device(d1, n)["by_reason"] == [n, 0, 0, 0]       # the ctx is as good as before
        assert cfg.g2_check_points_device(d2, n)["by_reason"] == [n, 0, 0, 0]
    finally:
        cfg.free(d1)
        cfg.free(d2)


# ---- 5. no side effects on the MSMs of the same ctx --------------------------------------------------------------------
def test_msm_results_unchanged_by_checks(cfg, msm_pkg):
    n = 1 << 12
    points, scalars = msm_pkg.generate_instance_host(c.o.SEED_BASE + 5, n)
    ks, dl = th.msm_case(64, 3)
    sc2, pts2 = th.encode_case(ks, dl, 0, 0)
    before, g2_before = cfg.msm(scalars, points, n), cfg.msm_g2(sc2, pts2, 64)
    assert cfg.check_points(points, n)[0]["n_invalid"] == 0
    assert cfg.g2_check_points(pts2, 64)[0]["n_invalid"] == 0
    assert cfg.g2_check_points(valid_g2(msm_pkg, 4099), 4099, reasons=False)[0]["n_invalid"] == 0
    assert cfg.msm(scalars, points, n) == before and cfg.msm_g2(sc2, pts2, 64) == g2_before


# ---- 6. the bounded wait -----------------------------------------------------------------------------------------------
def test_check_behind_a_held_stream_times_out_and_recovers(msm_pkg):
    n = 300
    g1, g2 = valid_g1(msm_pkg, n), valid_g2(msm_pkg, n)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no check buffer is sized yet
    try:
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)
        for fn, buf in ((c2.check_points, g1), (c2.g2_check_points, g2)):
            with pytest.raises(msm_pkg.MsmError) as e:
                fn(buf, n)
            assert e.value.status == msm_pkg.PIPELINE_ERROR and "check_points" in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.check_points(g1, n)[0]["by_reason"] == [n, 0, 0, 0]
        assert c2.g2_check_points(g2, n)[0]["by_reason"] == [n, 0, 0, 0]
    finally:
        c2.close()
