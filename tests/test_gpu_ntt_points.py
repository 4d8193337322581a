"""GPU tests of the transform over G1 points: the device entry, the host-buffer entry and the host twin byte for byte, and
against the model of ntt_points_ref -- every position up to log_n = 10 (7: one wave of butterflies, 8: the last level of
fewer than 64 blocks beside uniform ones, 9: one 256-lane block, 10: two), 32 sampled positions at log_n = 12; the planted
vectors at every level; prepared input and output, the output as the bases of an MSM; in place and out of place;
chunking; isolation from the MSM; the bounded wait.  Expected values come from the model, never from the library."""
import random

import pytest

import check_ref as c
import ntt_points_ref as npr
import ntt_ref
from test_ntt_points_host import check_positions, records

pytestmark = pytest.mark.gpu

F, I = npr.FORWARD, npr.INVERSE
o = c.o


def on_device(cfg, data):
    d = cfg.alloc(len(data))
    cfg.to_device(d, data)
    return d


def device_ntt(cfg, dom, data, direction, li, lo, n):
    size = 64 if lo == npr.PREPARED else npr.OUT_BYTES[lo]
    d_in, d_out = on_device(cfg, data), cfg.alloc(n * size)
    try:
        cfg.ntt_points_device(dom, d_in, d_out, direction, li, lo)
        assert cfg.to_host(d_in, len(data)) == data, "an out-of-place call changed its input"
        return cfg.to_host(d_out, n * size)
    finally:
        cfg.free(d_in)
        cfg.free(d_out)


def everywhere(cfg, msm_pkg, root, log_n, direction, data, li, lo):
    """device entry == host-buffer entry == host twin; returns the bytes"""
    dom = cfg.ntt_domain(root, log_n)
    try:
        h = msm_pkg.host_ntt_points(data, root, log_n, direction, li, lo)
        b = cfg.ntt_points(dom, data, direction, li, lo)
        d = device_ntt(cfg, dom, data, direction, li, lo, 1 << log_n)
    finally:
        dom.free()
    assert d == h, "device entry differs from the host twin"
    assert b == h, "host-buffer entry differs from the host twin"
    return d


@pytest.mark.parametrize("log_n", (0, 1, 2, 6, 7, 8, 9, 10))
def test_every_position(cfg, msm_pkg, log_n):
    a = list(npr.random_logs(log_n))
    k = log_n % 4
    li, lo = npr.IN_LAYOUTS[k], npr.OUT_LAYOUTS[log_n % 2]
    data = npr.in_records(a, li)
    for direction, root in ((F, npr.ARK if log_n % 2 else npr.H2C), (I, npr.H2C)):
        got = everywhere(cfg, msm_pkg, root, log_n, direction, data, li, lo)
        check_positions(got, npr.transform(a, root, log_n, direction), lo, (log_n, direction))


def test_sampled_positions_at_4096(cfg, msm_pkg):
    log_n, n = 12, 4096
    a = list(npr.random_logs(log_n))
    data = npr.in_records(a, c.H2C)
    got = everywhere(cfg, msm_pkg, npr.H2C, log_n, I, data, c.H2C, c.H2C)
    want = npr.transform(a, npr.H2C, log_n, I)
    recs = records(got, 64)
    for k in [0, 1, n - 1] + random.Random(12).sample(range(n), 29):
        assert recs[k] == npr.out_record(want[k], c.H2C), k


@pytest.mark.parametrize("log_n", (2, 7))
@pytest.mark.parametrize("direction", (F, I))
def test_planted_vectors_at_every_level(cfg, msm_pkg, direction, log_n):
    root = npr.H2C
    dom = cfg.ntt_domain(root, log_n)
    try:
        for name, a in npr.planted(root, log_n, direction).items():
            data = npr.in_records(a, c.H2C)
            for levels, state in enumerate(npr.level_states(a, root, log_n, direction)):
                got = cfg.test_ntt_points_levels(dom, data, levels, direction)
                assert got == msm_pkg.test_host_ntt_points_levels(data, root, log_n, levels, direction), (name, levels)
                check_positions(got, state, c.H2C, (name, direction, log_n, "levels", levels))
            got = cfg.ntt_points(dom, data, direction)
            check_positions(got, npr.transform(a, root, log_n, direction), c.H2C, (name, direction, log_n))
    finally:
        dom.free()


def test_prepared_input_and_output(cfg, msm_pkg):
    log_n, n, root = 8, 256, npr.H2C
    rng = random.Random(256)
    tau = rng.randrange(2, npr.R)
    srs = [pow(tau, j, npr.R) for j in range(n)]
    coeffs = [rng.randrange(npr.R) for _ in range(n)]
    prepared = msm_pkg.POINT_PREPARED
    dom = cfg.ntt_domain(root, log_n)
    d_srs = on_device(cfg, npr.in_records(srs, c.H2C))
    d_mono = cfg.bases_prepare_device(d_srs, n, c.H2C)                       # prepared records of [tau^j] G
    d_lag, d_aff = cfg.alloc(64 * n), cfg.alloc(72 * n)
    d_ev = on_device(cfg, msm_pkg.host_ntt(ntt_ref.encode(coeffs, 0), root, log_n, F))
    try:
        cfg.ntt_points_device(dom, d_mono, d_lag, I, prepared, prepared)     # prepared in, prepared out
        got = cfg.to_host(d_lag, 64 * n)
        lag = npr.lagrange_at(tau, root, log_n)
        for lo in npr.OUT_LAYOUTS:                                           # the bytes of the bases conversion
            cfg.ntt_points_device(dom, d_srs, d_aff, I, c.H2C, lo)
            aff = cfg.to_host(d_aff, npr.OUT_BYTES[lo] * n)
            check_positions(aff, lag, lo, ("lagrange", lo))
            d_ref = cfg.bases_prepare_device(d_aff, n, lo)
            try:
                assert cfg.to_host(d_ref, 64 * n) == got
            finally:
                cfg.free(d_ref)
        out = cfg.msm_batch_device([d_ev], [d_lag], [n], point_layout=prepared)[0]      # sum p(w^i) [L_i(tau)] G
    finally:
        dom.free()
        for p in (d_srs, d_mono, d_lag, d_aff, d_ev):
            cfg.free(p)
    p_tau = sum(cf * pow(tau, j, npr.R) for j, cf in enumerate(coeffs)) % npr.R
    assert o.decode_jacobian_mont_le(out) == npr.gmul(p_tau)


def test_in_place(cfg, msm_pkg):
    log_n, n = 7, 128
    a = list(npr.random_logs(log_n))
    dom = cfg.ntt_domain(npr.ARK, log_n)
    try:
        for li, lo in ((c.H2C, c.H2C), (c.JAC_BE32, c.ARK_AFFINE), (c.ARK_AFFINE, c.H2C)):
            data = npr.in_records(a, li)
            want = msm_pkg.host_ntt_points(data, npr.ARK, log_n, I, li, lo)
            d = on_device(cfg, data)
            try:
                cfg.ntt_points_device(dom, d, d, I, li, lo)
                assert cfg.to_host(d, n * npr.OUT_BYTES[lo]) == want, (li, lo)
            finally:
                cfg.free(d)
    finally:
        dom.free()


def test_chunked_call_writes_the_same_bytes(msm_pkg, monkeypatch):
    """MSM_AMD_MUL_CHUNK (read at msm_amd_init) at one normalisation group: every level of 64 butterflies runs in four
    chunks, the n^-1 pass in eight"""
    log_n = 7
    monkeypatch.setenv("MSM_AMD_MUL_CHUNK", "16")
    c2 = msm_pkg.setup_metal_state()
    try:
        a = list(npr.random_logs(log_n))
        data = npr.in_records(a, c.ARK_PROJECTIVE)
        for direction in (F, I):
            got = everywhere(c2, msm_pkg, npr.H2C, log_n, direction, data, c.ARK_PROJECTIVE, c.ARK_AFFINE)
            check_positions(got, npr.transform(a, npr.H2C, log_n, direction), c.ARK_AFFINE, ("chunked", direction))
    finally:
        c2.close()


def test_msm_before_and_after_and_stale_workspaces(cfg, msm_pkg):
    log_n, n = 6, 64
    a = list(npr.random_logs(log_n))
    data = npr.in_records(a, c.H2C)
    rng = random.Random(64)
    scalars = b"".join(o.encode_scalar_h2c(rng.randrange(npr.R)) for _ in range(n))
    points = npr.out_records(a, c.H2C)
    dom = cfg.ntt_domain(npr.H2C, log_n)
    try:
        before = msm_pkg.gpu_msm_h2c(scalars, points, cfg)
        first = cfg.ntt_points(dom, data, I)
        cfg.test_fill_workspaces(0xFF)
        assert cfg.ntt_points(dom, data, I) == first
        assert msm_pkg.gpu_msm_h2c(scalars, points, cfg) == before
    finally:
        dom.free()
    assert first == msm_pkg.host_ntt_points(data, npr.H2C, log_n, I)


def test_argument_errors(cfg, msm_pkg):
    def input_error(fn, *args, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*args, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    log_n, n = 3, 8
    data = npr.in_records(list(npr.random_logs(log_n)), c.H2C)
    dom, freed = cfg.ntt_domain(npr.H2C, log_n), cfg.ntt_domain(npr.H2C, log_n)
    freed.free()
    c2 = msm_pkg.setup_metal_state()
    d_in, d_out = on_device(cfg, data + bytes(96 * n)), cfg.alloc(96 * n)
    L = msm_pkg.lib()
    try:
        other = c2.ntt_domain(npr.H2C, log_n)
        for bad in (freed.h, other.h):
            assert L.msm_amd_ntt_points(cfg.h, bad, F, 0, data, 0, bytes(64 * n)) == msm_pkg.INPUT_ERROR
            assert L.msm_amd_ntt_points_device(cfg.h, bad, F, 0, d_in, 0, d_out, None) == msm_pkg.INPUT_ERROR
        assert L.msm_amd_ntt_points(None, dom.h, F, 0, data, 0, bytes(64 * n)) == msm_pkg.INPUT_ERROR
        input_error(cfg.ntt_points, dom, data, 2)
        input_error(cfg.ntt_points, dom, data, F, msm_pkg.POINT_PREPARED, 0)       # prepared on a host-buffer call
        input_error(cfg.ntt_points, dom, data, F, 0, msm_pkg.POINT_PREPARED)
        input_error(cfg.ntt_points, dom, data, F, msm_pkg.POINT_TABLES, 0)
        input_error(cfg.ntt_points, dom, data, F, 0, c.ARK_PROJECTIVE)
        input_error(cfg.ntt_points, dom, None, F)
        input_error(cfg.test_ntt_points_levels, dom, data, log_n + 1)
        input_error(cfg.ntt_points_device, dom, d_in, d_out, F, msm_pkg.POINT_TABLES, 0)
        input_error(cfg.ntt_points_device, dom, d_in, d_out, F, 0, msm_pkg.POINT_TABLES)
        input_error(cfg.ntt_points_device, dom, d_in, d_out, F, 9, 0)
        input_error(cfg.ntt_points_device, dom, d_in, d_out, -1, 0, 0)
        input_error(cfg.ntt_points_device, dom, None, d_out, F, 0, 0)
        input_error(cfg.ntt_points_device, dom, d_in, None, F, 0, 0)
        input_error(cfg.ntt_points_device, dom, d_in, d_in + 64, F, 0, 0)          # overlapping, not equal
        input_error(cfg.ntt_points_device, dom, d_in + 64, d_in, F, 0, 0)
        cfg.ntt_points_device(dom, d_in, d_in + 64 * n, F, 0, 0)                   # disjoint neighbours: fine
        assert cfg.to_host(d_in + 64 * n, 64 * n) == msm_pkg.host_ntt_points(data, npr.H2C, log_n, F)
    finally:
        c2.close()
        dom.free()
        cfg.free(d_in)
        cfg.free(d_out)


def test_behind_a_held_stream_times_out_and_recovers(msm_pkg):
    log_n = 4
    data = npr.in_records(list(npr.random_logs(log_n)), c.H2C)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of this call is sized yet
    try:
        dom = c2.ntt_domain(npr.H2C, log_n)
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)
        with pytest.raises(msm_pkg.MsmError) as e:
            c2.ntt_points(dom, data, I)
        assert e.value.status == msm_pkg.PIPELINE_ERROR and "msm_amd_ntt_points" in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.ntt_points(dom, data, I) == msm_pkg.host_ntt_points(data, npr.H2C, log_n, I)
    finally:
        c2.close()
