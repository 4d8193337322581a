"""The transform on the GPU (msm_amd_ntt_domain_*, msm_amd_ntt, msm_amd_ntt_device) against the host twin and the
big-integer model of tests/ntt_ref.py (tests/test_ntt_host.py pins the twin to the model on the CPU).  Every comparison is
of bytes.  The default plan cuts log_n levels into ceil(log_n / 10) passes: one up to 2^10, two up to 2^20, three from
2^21 on -- the largest pass count at or below 2^22, so 2^21 is the large size here."""
import ctypes
import random

import pytest

import ntt_ref as m

pytestmark = pytest.mark.gpu

R = m.R
BIG_LOG = 21


def on_device(cfg, data):
    d = cfg.alloc(max(32, len(data)))
    cfg.to_device(d, data)
    return d


def device_ntt(cfg, dom, data, direction, layout, shift, n_vec=1, in_place=False):
    """the device entry on freshly uploaded buffers; out of place: d_out pre-filled with 0xFF, d_in must survive"""
    d_in = on_device(cfg, data)
    d_out = d_in if in_place else on_device(cfg, b"\xFF" * len(data))
    try:
        cfg.ntt_device(dom, d_in, d_out, direction, layout, shift, n_vec)
        if not in_place:
            assert cfg.to_host(d_in, len(data)) == data
        return cfg.to_host(d_out, len(data))
    finally:
        cfg.free(d_in)
        if not in_place:
            cfg.free(d_out)


def first_difference(got, exp):
    assert len(got) == len(exp)
    for i in range(0, len(exp), 32):
        if got[i:i + 32] != exp[i:i + 32]:
            return "record %d: %s != %s" % (i // 32, got[i:i + 32].hex(), exp[i:i + 32].hex())
    return None


# ---- 1. all small sizes at the default tile ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(14))
def test_small_sizes(cfg, msm_pkg, log_n):
    n = 1 << log_n
    a = m.random_vector(300 + log_n, n)
    root = log_n & 1
    g = random.Random(log_n).randrange(1, R)
    dom = cfg.ntt_domain(root, log_n)
    try:
        info = dom.info()
        assert (info["root"], info["log_n"]) == (root, log_n)
        assert info["omega"] == m.encode([m.omega(root, log_n)], m.MONT_LE)
        assert 0 < info["device_bytes"] <= 32 * n
        for direction in m.DIRECTIONS:
            exp_values = m.transform(a, root, log_n, direction, g)
            for layout in m.LAYOUTS:
                data, shift, exp = m.encode(a, layout), m.shift_record(g, layout), m.encode(exp_values, layout)
                assert first_difference(msm_pkg.host_ntt(data, root, log_n, direction, layout, shift), exp) is None
                assert first_difference(device_ntt(cfg, dom, data, direction, layout, shift), exp) is None
                assert first_difference(cfg.ntt(dom, data, direction, layout, shift), exp) is None
    finally:
        dom.free()


# ---- 2. small tiles: one to five passes, every remainder ----------------------------------------------------------------------
@pytest.mark.parametrize("tile_log", [2, 3])
def test_small_tiles(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_NTT_TILE_LOG (read at msm_amd_init) lowers the tile to 4 or 8 elements: log_n 1 .. 9 are one to five passes
    of every length the plan can produce, on at most 512 elements; two vectors per call so that a tile index crosses a
    vector"""
    monkeypatch.setenv("MSM_AMD_NTT_TILE_LOG", str(tile_log))
    c2 = msm_pkg.setup_metal_state()
    try:
        for log_n in range(1, 10):
            n = 1 << log_n
            a = m.random_vector(700 + log_n, 2 * n)
            g = 5 + log_n
            dom = c2.ntt_domain(m.H2C, log_n)
            for direction in m.DIRECTIONS:
                layout = (log_n + direction) & 1
                exp = m.encode(m.transform(a[:n], m.H2C, log_n, direction, g) + m.transform(a[n:], m.H2C, log_n, direction, g), layout)
                data, shift = m.encode(a, layout), m.shift_record(g, layout)
                assert first_difference(device_ntt(c2, dom, data, direction, layout, shift, 2, in_place=bool(log_n & 1)), exp) is None, (log_n, direction)
                plain = m.encode(m.transform(a[:n], m.H2C, log_n, direction), layout)
                assert first_difference(c2.ntt(dom, data[:32 * n], direction, layout), plain) is None, (log_n, direction)
            dom.free()
    finally:
        c2.close()


# ---- 3. the first size of three passes --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_domain(cfg):
    dom = cfg.ntt_domain(m.ARK, BIG_LOG)
    yield dom
    dom.free()


def test_three_passes_dense(cfg, msm_pkg, big_domain):
    n = 1 << BIG_LOG
    raw = bytearray(random.Random(21).randbytes(32 * n))
    raw[31::32] = bytes(b & 0x1F for b in raw[31::32])    # every record < 2^253 < r: reduced MONT_LE records
    data = bytes(raw)
    shift = m.shift_record(7, m.MONT_LE)
    exp = msm_pkg.host_ntt(data, m.ARK, BIG_LOG, m.FORWARD, m.MONT_LE, shift)
    d_in, d_out = on_device(cfg, data), cfg.alloc(32 * n)
    try:
        cfg.ntt_device(big_domain, d_in, d_out, m.FORWARD, m.MONT_LE, shift)
        assert first_difference(cfg.to_host(d_out, 32 * n), exp) is None
        cfg.ntt_device(big_domain, d_out, d_out, m.INVERSE, m.MONT_LE, shift)          # the round trip, in place
        assert first_difference(cfg.to_host(d_out, 32 * n), data) is None
    finally:
        cfg.free(d_in)
        cfg.free(d_out)


def test_three_passes_sparse_closed_form(cfg, big_domain):
    n = 1 << BIG_LOG
    terms = [(1, 3), (n // 2 + 3, R - 5), (n - 1, 0x1234567890ABCDEF1234567890ABCDEF)]
    data = bytearray(32 * n)
    for i, c in terms:
        data[32 * i:32 * i + 32] = m.encode([c], m.CANON_LE)
    g = 11
    out = cfg.ntt(big_domain, bytes(data), m.FORWARD, m.CANON_LE, m.shift_record(g, m.CANON_LE))
    ks = sorted(set(random.Random(4096).sample(range(n), 4096)) | {0, n // 2, n - 1})
    for k in ks:
        assert out[32 * k:32 * k + 32] == m.encode([m.sparse_forward(terms, m.ARK, BIG_LOG, k, g)], m.CANON_LE), k


# ---- 4. batch and aliasing ----------------------------------------------------------------------------------------------------
def test_batch_and_aliasing(cfg, msm_pkg):
    log_n, n_vec = 11, 3
    n = 1 << log_n
    data = m.encode(m.random_vector(11, n_vec * n), m.MONT_LE)
    shift = m.shift_record(5, m.MONT_LE)
    dom = cfg.ntt_domain(m.H2C, log_n)
    d_in = on_device(cfg, data)
    try:
        for direction in m.DIRECTIONS:
            singles = b"".join(device_ntt(cfg, dom, data[32 * n * v:32 * n * (v + 1)], direction, m.MONT_LE, shift)
                               for v in range(n_vec))
            assert singles == msm_pkg.host_ntt(data, m.H2C, log_n, direction, m.MONT_LE, shift, n_vec)
            assert device_ntt(cfg, dom, data, direction, m.MONT_LE, shift, n_vec) == singles             # d_in survives
            assert device_ntt(cfg, dom, data, direction, m.MONT_LE, shift, n_vec, in_place=True) == singles
            assert cfg.ntt(dom, data, direction, m.MONT_LE, shift, n_vec) == singles
        for off in (32, 32 * n_vec * n - 32):   # d_out inside d_in's range, from either side
            for a, b in ((d_in, d_in + off), (d_in + off, d_in)):
                with pytest.raises(msm_pkg.MsmError) as e:
                    cfg.ntt_device(dom, a, b, m.FORWARD, m.MONT_LE, None, n_vec)
                assert e.value.status == msm_pkg.INPUT_ERROR, e.value
        assert cfg.to_host(d_in, len(data)) == data
    finally:
        cfg.free(d_in)
        dom.free()


# ---- 5. stale memory ----------------------------------------------------------------------------------------------------------
def test_stale_workspaces_change_nothing(cfg, msm_pkg):
    log_n = 12                                           # two passes: the ctx's pass buffer is in use
    data = m.encode(m.random_vector(12, 1 << log_n), m.CANON_LE)
    shift = m.shift_record(9, m.CANON_LE)
    dom = cfg.ntt_domain(m.ARK, log_n)
    try:
        first = device_ntt(cfg, dom, data, m.INVERSE, m.CANON_LE, shift)
        cfg.test_fill_workspaces(0xFF)
        assert device_ntt(cfg, dom, data, m.INVERSE, m.CANON_LE, shift) == first          # d_out pre-filled with 0xFF
        assert cfg.ntt(dom, data, m.INVERSE, m.CANON_LE, shift) == first
        assert first == msm_pkg.host_ntt(data, m.ARK, log_n, m.INVERSE, m.CANON_LE, shift)
    finally:
        dom.free()


# ---- 6. the output feeds the MSM ----------------------------------------------------------------------------------------------
def test_inverse_transform_feeds_the_msm(cfg, msm_pkg):
    log_n = 10
    n = 1 << log_n
    points, evals = msm_pkg.generate_instance_host(77, n)
    d_points, d_scalars = on_device(cfg, points), on_device(cfg, evals)
    dom = cfg.ntt_domain(m.H2C, log_n)
    try:
        cfg.ntt_device(dom, d_scalars, d_scalars, m.INVERSE, m.MONT_LE)
        out = ctypes.create_string_buffer(96)
        cfg._check(msm_pkg.lib().msm_amd_msm_device(cfg.h, msm_pkg.SCALAR_MONT_LE, msm_pkg.POINT_H2C_AFFINE,
                                                    ctypes.c_void_p(d_scalars), ctypes.c_void_p(d_points), n, out))
        coeffs = msm_pkg.host_ntt(evals, m.H2C, log_n, m.INVERSE, m.MONT_LE)
        assert coeffs != evals
        assert out.raw == cfg.msm(coeffs, points, n)
    finally:
        dom.free()
        cfg.free(d_points)
        cfg.free(d_scalars)


# ---- 7. the bounded wait, handles, arguments -----------------------------------------------------------------------------------
def test_ntt_behind_a_held_stream_times_out_and_recovers(msm_pkg):
    log_n = 11
    data = m.encode(m.random_vector(3, 1 << log_n), m.MONT_LE)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        dom = c2.ntt_domain(m.ARK, log_n)
        d = on_device(c2, data)
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        with pytest.raises(msm_pkg.MsmError) as e:
            c2.ntt_device(dom, d, d, m.FORWARD, m.MONT_LE)
        assert e.value.status == msm_pkg.PIPELINE_ERROR and "msm_amd_ntt_device" in str(e.value), e.value
        with pytest.raises(msm_pkg.MsmError) as e:
            c2.ntt(dom, data, m.FORWARD, m.MONT_LE)
        assert e.value.status == msm_pkg.PIPELINE_ERROR and "msm_amd_ntt" in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        exp = msm_pkg.host_ntt(data, m.ARK, log_n, m.FORWARD, m.MONT_LE)
        assert c2.to_host(d, len(data)) == data            # the refused calls wrote nothing
        c2.ntt_device(dom, d, d, m.FORWARD, m.MONT_LE)
        assert c2.to_host(d, len(data)) == exp
        assert c2.ntt(dom, data, m.FORWARD, m.MONT_LE) == exp
        c2.free(d)
    finally:
        c2.close()                                         # releases the domain the test did not free


def test_handles_and_argument_errors(cfg, msm_pkg):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    log_n = 4
    n = 1 << log_n
    data = m.encode(list(range(n)), m.CANON_LE)
    d_in, d_out = on_device(cfg, data), on_device(cfg, b"\xA5" * len(data))
    dom = cfg.ntt_domain(m.ARK, log_n)
    c2 = msm_pkg.setup_metal_state()
    points, _ = msm_pkg.generate_instance_host(5, 16)
    tables = cfg.tables_build(points, 16)
    try:
        other = c2.ntt_domain(m.ARK, log_n)
        input_error(cfg.ntt_device, other, d_in, d_out, 0, 1)                  # a domain of another ctx
        input_error(cfg.ntt, other, data, 0, 1)
        input_error(cfg.ntt_device, tables, d_in, d_out, 0, 1)                 # a table handle
        freed = cfg.ntt_domain(m.H2C, log_n)
        freed.free()
        input_error(cfg.ntt_device, freed, d_in, d_out, 0, 1)                  # a freed handle
        input_error(freed.info)
        input_error(freed.free)
        input_error(cfg.ntt_domain, 2, log_n)
        input_error(cfg.ntt_domain, m.ARK, 29)
        input_error(cfg.ntt_device, dom, d_in, d_out, 2, 1)                    # direction
        input_error(cfg.ntt_device, dom, d_in, d_out, 0, msm_pkg.SCALAR_CANON_BE32)
        input_error(cfg.ntt_device, dom, d_in, d_out, 0, 1, bytes(32))         # g = 0
        input_error(cfg.ntt_device, dom, d_in, d_out, 0, 1, m.encode([R], 1))  # g = r
        input_error(cfg.ntt_device, dom, None, d_out, 0, 1)
        input_error(cfg.ntt_device, dom, d_in, None, 0, 1)
        input_error(cfg.ntt_device, dom, d_in, d_out, 0, 1, None, 1 << 28)     # n_vec n = 2^32
        assert cfg.to_host(d_out, len(data)) == b"\xA5" * len(data)
        cfg.ntt_device(dom, None, None, 0, 1, None, 0)                         # n_vec = 0: OK, nothing touched
        assert cfg.to_host(d_out, len(data)) == b"\xA5" * len(data)
        cfg.ntt_device(dom, d_in, d_out, 0, 1)                                 # the ctx is as good as before
        assert cfg.to_host(d_out, len(data)) == m.encode(m.naive(list(range(n)), m.ARK, log_n, m.FORWARD), m.CANON_LE)
        other.free()
    finally:
        c2.close()
        cfg.tables_free(tables)
        dom.free()
        cfg.free(d_in)
        cfg.free(d_out)
