"""GPU tests of the compressed point formats: the decompress / compress kernels against their host twins byte for byte
and against the big-integer model of compress_ref at the planted records, over lane tails, wave and workgroup
boundaries; prepared output against the bases conversion and in an MSM; the subgroup recipe; the report; the raw root
ops; isolation from the MSMs of the same ctx; the bounded wait; no scratch."""
import random

import pytest

import check_ref as c
import compress_ref as r
import g2_ref as g
import test_compress_host as hst
import test_g2_host as th

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
FORMATS = [r.ARK, r.PARITY]
LAYOUTS = hst.LAYOUTS
_VALID = {}


def on_device(cfg, data):
    d = cfg.alloc(len(data))
    cfg.to_device(d, data)
    return d


def drop_ms(rep):
    return {k: v for k, v in rep.items() if k != "device_ms"}


def valid_compressed(msm_pkg, group, fmt, n):
    """n valid points from the library's generators, compressed by the host twin (itself checked against the model in
    test_compress_host); computed once per (group, format)"""
    key = (group, fmt)
    if key not in _VALID:
        m = max(SIZES)
        if group == 1:
            pts = msm_pkg.generate_instance_host(c.o.SEED_BASE + 91, m)[0]
        else:
            pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(90001, g.GEN2)), g.encode_h2c(g.scalar_mul(7919, g.GEN2)), m)
        data, bad = msm_pkg.host_compress_points(pts, m, fmt, 0, g2=group == 2)
        assert bad == 0
        _VALID[key] = (data, pts)
    data, pts = _VALID[key]
    return data[:n * r.SIZE[group]], pts[:n * (64 if group == 1 else 128)]


def decompress_everywhere(cfg, msm_pkg, group, fmt, layout, buf, n, placed):
    """device entry == host-buffer entry == host twin, and all equal the model at the planted records"""
    g2 = group == 2
    h_out, h_rep, h_reasons = msm_pkg.host_decompress_points(buf, n, fmt, layout, g2=g2)
    b_out, b_rep, b_reasons = cfg.decompress_points(buf, n, fmt, layout, g2=g2)
    size = msm_pkg.decompressed_bytes(layout, g2)
    d_in, d_out, d_rs = on_device(cfg, buf), cfg.alloc(n * size), cfg.alloc(n)
    try:
        d_rep = cfg.decompress_points_device(d_in, n, d_out, fmt, layout, g2=g2, d_reasons=d_rs)
        d_bytes, d_reasons = cfg.to_host(d_out, n * size), cfg.to_host(d_rs, n)
        d_rep_null = cfg.decompress_points_device(d_in, n, d_out, fmt, layout, g2=g2)       # d_reasons == NULL
    finally:
        for p in (d_in, d_out, d_rs):
            cfg.free(p)
    assert d_reasons == h_reasons == b_reasons
    assert d_bytes == h_out and b_out == h_out
    assert drop_ms(d_rep) == drop_ms(h_rep) == drop_ms(b_rep) == drop_ms(d_rep_null), (d_rep, h_rep, b_rep)
    assert d_rep["device_ms"] > 0 and sum(d_rep["by_reason"]) == n == d_rep["n_checked"]
    for i, rec in placed.items():
        reason, pt = r.decode(group, fmt, rec)
        assert d_reasons[i] == reason, i
        assert d_bytes[i * size:(i + 1) * size] == r.out_record(group, layout, pt), i
    bad = [i for i, rec in placed.items() if r.expected_reason(group, fmt, rec)]
    assert d_rep["n_invalid"] == len(bad) == n - d_reasons.count(0)                          # nothing but the planted ones
    assert d_rep["first_invalid"] == (min(bad) if bad else None)
    assert d_rep["n_identity"] == sum(r.is_identity(group, fmt, rec) for rec in placed.values())
    return d_rep


# ---- 1. device against host twin and model ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_decompress_sizes(cfg, msm_pkg, group, n):
    k = SIZES.index(n)
    fmt, layout = FORMATS[k % 2], LAYOUTS[group][(k // 2) % 2]
    cases, _ = r.case_records(group, fmt, n)
    buf, placed = r.plant(valid_compressed(msm_pkg, group, fmt, n)[0], r.SIZE[group], cases, n, random.Random(n))
    decompress_everywhere(cfg, msm_pkg, group, fmt, layout, buf, n, placed)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decompress_every_layout(cfg, msm_pkg, group, fmt):
    n = 257
    cases, _ = r.case_records(group, fmt, 3)
    buf, placed = r.plant(valid_compressed(msm_pkg, group, fmt, n)[0], r.SIZE[group], cases, n, random.Random(fmt))
    for layout in LAYOUTS[group]:
        decompress_everywhere(cfg, msm_pkg, group, fmt, layout, buf, n, placed)


# ---- 2. prepared output ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_prepared_output_equals_the_bases_conversion(cfg, msm_pkg, group, fmt):
    n, g2 = 257, group == 2
    cases, _ = r.case_records(group, fmt, 4)
    buf, _ = r.plant(valid_compressed(msm_pkg, group, fmt, n)[0], r.SIZE[group], cases, n, random.Random(8))
    prepared = msm_pkg.G2_POINT_PREPARED if g2 else msm_pkg.POINT_PREPARED
    psize = msm_pkg.decompressed_bytes(prepared, g2)
    d_in, d_prep = on_device(cfg, buf), cfg.alloc(n * psize)
    try:
        rep = cfg.decompress_points_device(d_in, n, d_prep, fmt, prepared, g2=g2)
        got = cfg.to_host(d_prep, n * psize)
        for layout in LAYOUTS[group]:                                     # both affine forms convert to the same records
            asize = msm_pkg.decompressed_bytes(layout, g2)
            d_aff = cfg.alloc(n * asize)
            try:
                rep_a = cfg.decompress_points_device(d_in, n, d_aff, fmt, layout, g2=g2)
                d_ref = (cfg.g2_bases_prepare_device if g2 else cfg.bases_prepare_device)(d_aff, n, layout)
                try:
                    assert cfg.to_host(d_ref, n * psize) == got
                finally:
                    cfg.free(d_ref)
            finally:
                cfg.free(d_aff)
            assert drop_ms(rep_a) == drop_ms(rep)
    finally:
        cfg.free(d_in)
        cfg.free(d_prep)
    assert rep["n_invalid"] > 0 and rep["n_identity"] == 1


def test_msm_over_decompressed_prepared_bases_g1(cfg, msm_pkg):
    n = 257
    rng = random.Random(21)
    dl = [rng.randrange(1, 1 << 40) for _ in range(n)]
    ks = [rng.randrange(c.R_ORDER) for _ in range(n)]
    dl[3], ks[5] = 0, 0                                                   # an identity base, a zero scalar
    pts = [c.o.scalar_mul(a, c.o.GEN) if a else None for a in dl]
    scalars = b"".join(c.o.encode_scalar_h2c(k) for k in ks)
    want = c.o.scalar_mul(sum(k * a for k, a in zip(ks, dl)) % c.R_ORDER, c.o.GEN)
    plain = cfg.msm(scalars, b"".join(c.g1_rec(c.H2C, p).encode() for p in pts), n)
    assert c.o.decode_jacobian_mont_le(plain) == want
    for fmt in FORMATS:
        d_in = on_device(cfg, b"".join(r.encode(1, fmt, p) for p in pts))
        d_prep, d_sc = cfg.alloc(64 * n), on_device(cfg, scalars)
        try:
            assert cfg.decompress_points_device(d_in, n, d_prep, fmt, msm_pkg.POINT_PREPARED)["n_invalid"] == 0
            out = cfg.msm_batch_device([d_sc], [d_prep], [n], point_layout=msm_pkg.POINT_PREPARED)[0]
        finally:
            for p in (d_in, d_prep, d_sc):
                cfg.free(p)
        assert out == plain and c.o.decode_jacobian_mont_le(out) == want


def test_msm_over_decompressed_prepared_bases_g2(cfg, msm_pkg):
    n = 257
    ks, dl = th.msm_case(n, 5)
    sc, pts_bytes = th.encode_case(ks, dl, 0, 0)
    plain = cfg.msm_g2(sc, pts_bytes, n)
    th.assert_result(plain, th.expected(ks, dl))
    for fmt in FORMATS:
        d_in = on_device(cfg, b"".join(r.encode(2, fmt, th._point(a) if a else None) for a in dl))
        d_prep, d_sc = cfg.alloc(128 * n), on_device(cfg, sc)
        try:
            rep = cfg.decompress_points_device(d_in, n, d_prep, fmt, msm_pkg.G2_POINT_PREPARED, g2=True)
            assert rep["n_invalid"] == 0 and rep["n_identity"] == dl.count(0)
            out = cfg.msm_g2_device(d_sc, d_prep, n, point_layout=msm_pkg.G2_POINT_PREPARED)
        finally:
            for p in (d_in, d_prep, d_sc):
                cfg.free(p)
        assert out == plain
        th.assert_result(out, th.expected(ks, dl))


# ---- 3. the subgroup recipe: decompress, then check -------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_subgroup_recipe(cfg, msm_pkg, fmt):
    n = 65
    sp = c.special_g2()
    buf = bytearray(valid_compressed(msm_pkg, 2, fmt, n)[0])
    planted = {0: sp["curve"], 40: sp["g2_plus_cofactor"], 64: sp["curve"]}
    for i, pt in planted.items():
        buf[64 * i:64 * i + 64] = r.encode(2, fmt, pt)
    d_in, d_out, d_rs = on_device(cfg, bytes(buf)), cfg.alloc(128 * n), cfg.alloc(n)
    try:
        rep = cfg.decompress_points_device(d_in, n, d_out, fmt, msm_pkg.G2_POINT_H2C_AFFINE, g2=True)
        assert rep["by_reason"] == [n, 0, 0, 0, 0]                        # all VALID: no subgroup rule here
        out = cfg.to_host(d_out, 128 * n)
        for i, pt in planted.items():
            assert out[128 * i:128 * i + 128] == g.encode_h2c(pt)
        chk = cfg.g2_check_points_device(d_out, n, checks=msm_pkg.CHECK_CURVE | msm_pkg.CHECK_SUBGROUP, d_reasons=d_rs)
        reasons = cfg.to_host(d_rs, n)
    finally:
        for p in (d_in, d_out, d_rs):
            cfg.free(p)
    assert chk["by_reason"] == [n - 3, 0, 0, 3] and chk["first_invalid"] == 0
    assert [i for i in range(n) if reasons[i]] == sorted(planted) and all(reasons[i] == 3 for i in planted)


# ---- 4. the report ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_first_invalid_across_workgroups(cfg, msm_pkg, group):
    """The offender with the HIGHER index is rejected at once (both flag bits), the lower one only after the root
    ladder: first_invalid must still be the lower index."""
    n, fmt = 4099, r.ARK
    buf = bytearray(valid_compressed(msm_pkg, group, fmt, n)[0])
    size = r.SIZE[group]
    fast = r.raw_record(group, 5 if group == 1 else (5, 0), 0xC0)
    slow = r.raw_record(group, r.find_x(group, False, 77), 0)
    ident = r.encode(group, fmt, None)
    placed = {4098: fast, 70: slow, 1000: ident, 3000: ident}
    for i, rec in placed.items():
        buf[size * i:size * i + size] = rec
    rep = decompress_everywhere(cfg, msm_pkg, group, fmt, LAYOUTS[group][0], bytes(buf), n, placed)
    assert rep["first_invalid"] == 70 and rep["first_reason"] == r.NOT_ON_CURVE
    assert rep["by_reason"] == [n - 2, 0, 1, 0, 1] and rep["n_identity"] == 2


# ---- 5. compress ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_compress_device_against_host_twin(cfg, msm_pkg, group, n):
    g2 = group == 2
    k = SIZES.index(n)
    fmt, layout = FORMATS[k % 2], LAYOUTS[group][(k // 2) % 2]
    stride = msm_pkg.decompressed_bytes(layout, g2)
    h2c = valid_compressed(msm_pkg, group, fmt, n)[1]
    hsize = 64 if group == 1 else 128
    recs = [h2c[i * hsize:(i + 1) * hsize] + bytes(stride - hsize) for i in range(n)]
    mk = c.g1_rec if group == 1 else c.g2_rec
    pt = r.points(group, 1, 9)[0]
    planted = {0: c.non_reduced(mk(layout, pt), 0), n - 1: mk(layout, None)}
    if n > 64:
        planted[64] = c.non_reduced(mk(layout, pt), 1, top=True)
        planted[n // 2] = mk(layout, pt)
    for i, rec in planted.items():
        recs[i] = rec.encode()
    buf = b"".join(recs)
    h_out, h_bad = msm_pkg.host_compress_points(buf, n, fmt, layout, g2=g2)
    b_out, b_bad = cfg.compress_points(buf, n, fmt, layout, g2=g2)
    d_in, d_out = on_device(cfg, buf), cfg.alloc(n * r.SIZE[group])
    try:
        d_bad = cfg.compress_points_device(d_in, n, d_out, fmt, layout, g2=g2)
        d_bytes = cfg.to_host(d_out, n * r.SIZE[group])
    finally:
        cfg.free(d_in)
        cfg.free(d_out)
    assert d_bytes == h_out == b_out
    want = {i: r.compress_expected(group, fmt, rec) for i, rec in planted.items()}
    assert d_bad == h_bad == b_bad == sum(w[1] for w in want.values())
    for i, (rec, bad) in want.items():
        assert d_bytes[i * r.SIZE[group]:(i + 1) * r.SIZE[group]] == (b"\xff" * r.SIZE[group] if bad else rec)
    untouched = [i for i in range(n) if i not in planted]                  # the rest round-trips
    ref = valid_compressed(msm_pkg, group, fmt, n)[0]
    assert all(d_bytes[i * r.SIZE[group]:(i + 1) * r.SIZE[group]] == ref[i * r.SIZE[group]:(i + 1) * r.SIZE[group]]
               for i in untouched)


# ---- 6. the raw root ops ------------------------------------------------------------------------------------------------------
def test_raw_root_ops_device_equals_host(cfg, msm_pkg):
    ops, a = hst.fq_sqrt_inputs()
    dev = cfg.test_op_raw(msm_pkg.RAW_FE_SQRT, a, [0] * len(a), len(ops))
    assert dev == msm_pkg.test_op_raw_host(msm_pkg.RAW_FE_SQRT, a, [0] * len(a), len(ops))
    hst.check_fq_sqrt(ops, dev)
    ops2, a2 = hst.fq2_sqrt_inputs()
    dev2 = cfg.test_op_g2(msm_pkg.G2_RAW_FQ2_SQRT, a2, [0] * len(a2), len(ops2))
    assert dev2 == msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_FQ2_SQRT, a2, [0] * len(a2), len(ops2))
    assert hst.check_fq2_sqrt(ops2, dev2) == 7 + 64


# ---- 7. errors, isolation, the bounded wait -------------------------------------------------------------------------------------
def test_argument_errors(cfg, msm_pkg):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    n = 64
    g1, g2 = valid_compressed(msm_pkg, 1, 0, n)[0], valid_compressed(msm_pkg, 2, 0, n)[0]
    d1, d2, d_out = on_device(cfg, g1), on_device(cfg, g2), cfg.alloc(136 * n)
    try:
        for layout in (msm_pkg.POINT_ARK_PROJECTIVE, msm_pkg.POINT_JAC_BE32, msm_pkg.POINT_TABLES, 9):
            input_error(cfg.decompress_points_device, d1, n, d_out, 0, layout)
        input_error(cfg.decompress_points_device, d2, n, d_out, 0, msm_pkg.G2_POINT_TABLES, g2=True)
        input_error(cfg.decompress_points_device, d1, n, d_out, 2, msm_pkg.POINT_H2C_AFFINE)
        input_error(cfg.decompress_points_device, None, n, d_out, 0, msm_pkg.POINT_H2C_AFFINE)
        input_error(cfg.decompress_points_device, d1, n, None, 0, msm_pkg.POINT_H2C_AFFINE)
        input_error(cfg.decompress_points_device, d1, 1 << 32, d_out, 0, msm_pkg.POINT_H2C_AFFINE)
        L, rep = msm_pkg.lib(), msm_pkg.DecompressReport()
        import ctypes
        out = ctypes.create_string_buffer(136 * n)
        assert L.msm_amd_decompress_points(cfg.h, 0, g1, n, msm_pkg.POINT_PREPARED, out, None, ctypes.byref(rep)) == msm_pkg.INPUT_ERROR
        assert L.msm_amd_g2_decompress_points(cfg.h, 0, g2, n, msm_pkg.G2_POINT_PREPARED, out, None, ctypes.byref(rep)) == msm_pkg.INPUT_ERROR
        assert L.msm_amd_decompress_points(cfg.h, 0, g1, n, 0, out, None, None) == msm_pkg.INPUT_ERROR
        for layout in (msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, msm_pkg.POINT_JAC_BE32):
            input_error(cfg.compress_points_device, d_out, n, d1, 0, layout)
        input_error(cfg.compress_points_device, d_out, n, d2, 0, msm_pkg.G2_POINT_PREPARED, g2=True)
        input_error(cfg.compress_points_device, d_out, n, d1, 5, 0)
        for g2_ in (False, True):                                                            # n == 0: OK, an empty report
            rep0 = cfg.decompress_points_device(None, 0, None, 0, 0, g2=g2_)
            assert rep0["n_checked"] == 0 and rep0["first_invalid"] is None and rep0["by_reason"] == [0] * 5
            assert cfg.decompress_points(None, 0, 0, 0, g2=g2_)[1]["n_checked"] == 0
            assert cfg.compress_points_device(None, 0, None, 0, 0, g2=g2_) == 0
        assert cfg.decompress_points_device(d1, n, d_out, 0, 0)["by_reason"] == [n, 0, 0, 0, 0]     # the ctx is as good as before
        assert cfg.decompress_points_device(d2, n, d_out, 0, 0, g2=True)["by_reason"] == [n, 0, 0, 0, 0]
    finally:
        for p in (d1, d2, d_out):
            cfg.free(p)


def test_msm_results_unchanged_and_batch_in_flight(cfg, msm_pkg):
    n = 1 << 12
    points, scalars = msm_pkg.generate_instance_host(c.o.SEED_BASE + 5, n)
    ks, dl = th.msm_case(64, 3)
    sc2, pts2 = th.encode_case(ks, dl, 0, 0)
    before, g2_before = cfg.msm(scalars, points, n), cfg.msm_g2(sc2, pts2, 64)
    c1, c2 = valid_compressed(msm_pkg, 1, 1, 4099)[0], valid_compressed(msm_pkg, 2, 0, 257)[0]
    assert cfg.decompress_points(c1, 4099, 1, 0)[1]["n_invalid"] == 0
    assert cfg.decompress_points(c2, 257, 0, 1, g2=True)[1]["n_invalid"] == 0
    assert cfg.msm(scalars, points, n) == before and cfg.msm_g2(sc2, pts2, 64) == g2_before
    # a G1 batch submitted, a decompress call made, then the batch waited for
    dp, ds = on_device(cfg, points), on_device(cfg, scalars)
    try:
        handle = cfg.submit_batch_device([ds], [dp], [n])
        got = cfg.decompress_points(c1, 4099, 1, 0)
        res = cfg.wait_batch(handle)
    finally:
        cfg.free(dp)
        cfg.free(ds)
    assert got[1]["n_invalid"] == 0 and got[0] == msm_pkg.host_decompress_points(c1, 4099, 1, 0)[0]
    assert res[0] == before


def test_decompress_behind_a_held_stream_times_out_and_recovers(msm_pkg):
    n = 300
    g1, g2 = valid_compressed(msm_pkg, 1, 0, n)[0], valid_compressed(msm_pkg, 2, 0, n)[0]
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)
        for buf, is_g2 in ((g1, False), (g2, True)):
            with pytest.raises(msm_pkg.MsmError) as e:
                c2.decompress_points(buf, n, 0, 0, g2=is_g2)
            assert e.value.status == msm_pkg.PIPELINE_ERROR and "decompress_points" in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.decompress_points(g1, n, 0, 0)[1]["by_reason"] == [n, 0, 0, 0, 0]
        assert c2.decompress_points(g2, n, 0, 0, g2=True)[1]["by_reason"] == [n, 0, 0, 0, 0]
    finally:
        c2.close()


# ---- 8. resources ---------------------------------------------------------------------------------------------------------------
def test_compress_kernels_use_no_scratch():
    hst.test_compress_kernels_use_no_scratch()
