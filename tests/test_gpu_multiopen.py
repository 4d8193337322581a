"""The multi-point polynomial calls on the GPU (msm_amd_fr_poly_eval_points, msm_amd_fr_poly_div_points) against the host
twins and the big-integer model of tests/multiopen_ref.py (tests/test_multiopen_host.py pins the twins to the model on the
CPU).  Every comparison is of bytes: device call = host-buffer call (mem HOST) = twin = model -- partial fractions on the
device, chained linear divisions in the twin, schoolbook long division in the model.  The kernels work on the tiles and
levels of the single-point calls (2^T records, T = 9): sizes sit on both sides of a tile and of a level,
MSM_AMD_FR_TILE_LOG brings five levels down to a few hundred records."""
import ctypes
import random

import pytest

import mul_ref
import multiopen_ref as m
import poly_ref as p
from guard import Arena, At, HostArena, In, Out, guarded
from oracle import bn254_ref as o

pytestmark = pytest.mark.gpu

R = m.R
T = 9
TILE = 1 << T
BIG = 1 << 20
HOST, DEVICE = m.MEM_HOST, m.MEM_DEVICE
_POOL = {}


def pool(n):
    """the first n of 2 (2^18 + 8) random values, drawn once"""
    if not _POOL:
        _POOL["v"] = m.random_values(2025, 2 * ((1 << 18) + 8))
    return _POOL["v"][:n]


class Device:
    """device buffers of one test, freed together"""

    def __init__(self, cfg):
        self.cfg, self.ptrs = cfg, []

    def put(self, data):
        d = self.cfg.alloc(max(32, len(data)))
        self.ptrs.append(d)
        self.cfg.to_device(d, data)
        return d

    def get(self, d, nbytes):
        return self.cfg.to_host(d, nbytes)

    def close(self):
        for d in self.ptrs:
            self.cfg.free(d)
        self.ptrs = []


@pytest.fixture
def dev(cfg):
    d = Device(cfg)
    yield d
    d.close()


def device_div(dev, data, z, layout, n_vec, in_place, vals=True):
    """the division on fresh device buffers: out of place into 0xFF bytes, and the input must survive"""
    n = len(data) // 32 // n_vec
    d_in = dev.put(data)
    d_out = d_in if in_place else dev.put(b"\xFF" * len(data))
    _, val, ms = dev.cfg.fr_poly_div_points(d_in, z, layout, n_vec, DEVICE, n, d_out, vals)
    assert ms >= 0
    if not in_place:
        assert dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, len(data))
    dev.close()
    return out, val


def device_eval(dev, data, z, layout, n_vec):
    d_in = dev.put(data)
    y, ms = dev.cfg.fr_poly_eval_points(d_in, z, layout, n_vec, DEVICE, len(data) // 32 // n_vec)
    assert ms >= 0 and dev.get(d_in, len(data)) == data
    dev.close()
    return y


def check_points(cfg, msm_pkg, dev, data, z, layout, n_vec, tag, in_place=(False,), model=None):
    """evaluation and division: device call = host-buffer call = twin = model"""
    exp_q, exp_vals = model or m.div_points(data, z, layout, n_vec)
    q, vals = msm_pkg.host_fr_poly_div_points(data, z, layout, n_vec)
    assert m.first_difference(q, exp_q) is None and vals == exp_vals, tag
    assert msm_pkg.host_fr_poly_eval_points(data, z, layout, n_vec) == exp_vals, tag
    for ip in in_place:
        q, vals = device_div(dev, data, z, layout, n_vec, ip)
        assert m.first_difference(q, exp_q) is None, (tag, ip)
        assert vals == exp_vals, (tag, ip)
    assert device_eval(dev, data, z, layout, n_vec) == exp_vals, tag
    q, vals, _ = cfg.fr_poly_div_points(data, z, layout, n_vec)
    assert m.first_difference(q, exp_q) is None and vals == exp_vals, tag
    assert cfg.fr_poly_eval_points(data, z, layout, n_vec)[0] == exp_vals, tag


# ---- 1. small tiles: up to five levels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_log", [2, 3])
def test_small_tiles(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_FR_TILE_LOG (read at msm_amd_init) lowers the tile to 4 or 8 records; k cycles through 1 .. 8 so that
    every k meets several sizes, n < k among them"""
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", str(tile_log))
    c2 = msm_pkg.setup_metal_state()
    dev = Device(c2)
    try:
        assert msm_pkg.test_fr_poly_points_plan(513, 3, 8, tile_log)["levels"] == (5 if tile_log == 2 else 4)
        for idx, n in enumerate(list(range(1, 71)) + [257, 513]):
            layout = n & 1
            for n_vec in (1, 3):
                k = 1 + (idx * 3 + n_vec + tile_log) % 8
                data = m.encode(m.random_values(1000 * n_vec + n, n * n_vec), layout)
                name, z = m.point_sets(layout, k, n)[(n + n_vec) % 4]
                check_points(c2, msm_pkg, dev, data, z, layout, n_vec, (n, n_vec, k, name), (bool((n + n_vec) & 2),))
    finally:
        dev.close()
        c2.close()


# ---- 2. the default tile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("n", [63, 64, 65, 511, 512, 513, 1 << 18, (1 << 18) + 1])
def test_default_tile(cfg, msm_pkg, dev, n, k):
    """2^18 + 1 is the first size of three levels, and its top tile holds two records"""
    n_vec = 2 if n <= 513 else 1
    levels = msm_pkg.test_fr_poly_points_plan(n, n_vec, k, T)["levels"]
    assert levels == (1 if n <= TILE else 2 if n <= TILE * TILE else 3)
    layout = (n + k) & 1
    data = m.encode(pool(n * n_vec), layout)
    sets = m.point_sets(layout, k, n)
    for name, z in (sets if n <= 513 else sets[2:3]):
        check_points(cfg, msm_pkg, dev, data, z, layout, n_vec, (n, k, name), (False, True) if name == "rotations" else (False,))
    if n <= 513:   # unreduced words
        words = [((3 * i + 1) * R // 7 + i) % (1 << 256) for i in range(n * n_vec)]
        check_points(cfg, msm_pkg, dev, m.raw(words), sets[0][1], layout, n_vec, (n, k, "unreduced"))


def test_large_division_of_all_ones(cfg, msm_pkg, dev):
    """(1 + X + .. + X^(n-1)) div (X^2 - 1): q_i = floor((n - i - 1) / 2), at every tile edge of the first level"""
    n, layout = BIG, m.MONT_LE
    z = m.encode([1, R - 1], layout)
    data = m.encode([1], layout) * n
    exp_q, exp_vals = msm_pkg.host_fr_poly_div_points(data, z, layout, 1, 16)
    d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
    _, vals, ms = cfg.fr_poly_div_points(d_in, z, layout, 1, DEVICE, n, d_out)
    out = dev.get(d_out, len(data))
    assert ms > 0 and m.first_difference(out, exp_q) is None and vals == exp_vals == m.encode([n, 0], layout)
    y, ms = cfg.fr_poly_eval_points(d_in, z, layout, 1, DEVICE, n)
    assert ms > 0 and y == vals
    fixed = [0, 1, 63, 64, TILE - 1, TILE, TILE * TILE - 1, TILE * TILE, n // 2, n - TILE - 1, n - TILE, n - 3, n - 2, n - 1]
    fixed += random.Random(5).sample(range(n), 64 - len(fixed))
    edges = {e for b in range(1, n // TILE) for e in (b * TILE - 1, b * TILE)}
    for i in sorted(set(fixed) | edges):
        assert out[32 * i:32 * i + 32] == m.encode([(n - i - 1) // 2], layout), i
    assert out[32 * (n - 2):] == bytes(64)


# ---- 3. one point, special points, n < k ---------------------------------------------------------------------------------------
def test_one_point_is_the_single_point_call(cfg, msm_pkg, dev):
    for n in (1, 65, 513, TILE * TILE + 5):
        layout = n & 1
        data = m.encode(pool(2 * n), layout)
        for name, z in p.special_points(layout)[5:] if n > 513 else p.special_points(layout):
            d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
            rem, _ = cfg.fr_poly_div_linear_device(d_in, n, d_out, z, layout, 2)
            single = dev.get(d_out, len(data))
            assert cfg.fr_poly_eval_device(d_in, n, z, layout, 2)[0] == rem, (n, name)
            dev.close()
            assert device_div(dev, data, z, layout, 2, False) == (single, rem), (n, name)
            assert device_eval(dev, data, z, layout, 2) == rem, (n, name)


def test_special_points_and_the_refused_pair(cfg, msm_pkg, dev):
    n = TILE + 9
    for layout in m.LAYOUTS:
        data = m.encode(pool(n), layout)
        specials = [rec for _, rec in p.special_points(layout)]
        # zero / r and one / r + 1 are the same points: one of each
        z = specials[0] + specials[4] + specials[2] + specials[5] + specials[6]
        check_points(cfg, msm_pkg, dev, data, z, layout, 1, (layout, "specials"), (False, True))
        every = b"".join(specials)                                           # the evaluation takes repeated points
        assert device_eval(dev, data, every, layout, 1) == cfg.fr_poly_eval_points(data, every, layout)[0] == m.eval_points(data, every, layout)
        pair = m.raw([1]) + specials[6] + m.raw([R + 1])
        d_in, d_out = dev.put(data), dev.put(b"\xA5" * len(data))
        for call in (lambda: cfg.fr_poly_div_points(d_in, pair, layout, 1, DEVICE, n, d_out),
                     lambda: cfg.fr_poly_div_points(data, pair, layout)):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.INPUT_ERROR
            text = str(e.value)
            assert "msm_amd_fr_poly_div_points" in text and "points 0 and 2" in text, text
        assert dev.get(d_out, len(data)) == b"\xA5" * len(data) and dev.get(d_in, len(data)) == data
        dev.close()


def test_fewer_coefficients_than_points(cfg, msm_pkg, dev):
    for n, k in ((1, 2), (1, 8), (3, 4), (7, 8), (5, 5)):
        for layout in m.LAYOUTS:
            data = m.encode(m.random_values(n * k, 3 * n), layout)
            z = m.point_sets(layout, k, n)[1][1]
            check_points(cfg, msm_pkg, dev, data, z, layout, 3, (n, k), (False, True))
            assert device_div(dev, data, z, layout, 3, False)[0] == bytes(len(data))


# ---- 4. open a rotation set, on the device from the first call to the last -----------------------------------------------------
def test_multiopen_chain(cfg, msm_pkg, dev):
    """f = p_0 + x p_1 + x^2 p_2, q = f div Z_S in place (no subtraction of r(X)), [q(tau)]G by the MSM on the same pointer"""
    n, layout, k = 1 << 10, m.MONT_LE, 3
    rng = random.Random(32)
    tau, xv = rng.randrange(2, R), rng.randrange(R)
    psize = msm_pkg.decompressed_bytes(msm_pkg.POINT_PREPARED, False)
    d_tau = dev.put(mul_ref.scalars_bytes([pow(tau, i, R) for i in range(n)], 0))
    d_gen = dev.put(mul_ref.base_record(1, 0, mul_ref.GEN[1]))
    d_bases = dev.put(bytes(n * psize))
    cfg.mul_points_device(d_tau, d_gen, n, d_bases, msm_pkg.MUL_BASE_ONE, 0, 0, msm_pkg.POINT_PREPARED)     # [tau^i]G
    polys = m.random_values(33, 3 * n)
    name, z = m.point_sets(layout, k, 5)[2]
    zs = m.point_values(z, layout)
    d_p = dev.put(m.encode(polys, layout))
    cfg.fr_lincomb_device(d_p, n, d_p, m.encode([xv], layout), layout, 3)
    _, vals, _ = cfg.fr_poly_div_points(d_p, z, layout, 1, DEVICE, n, d_p)
    out = ctypes.create_string_buffer(96)
    vp = ctypes.c_void_p
    assert msm_pkg.lib().msm_amd_msm_device(cfg.h, layout, msm_pkg.POINT_PREPARED, vp(d_p), vp(d_bases), n, out) == msm_pkg.OK
    f = [(polys[i] + xv * polys[n + i] + xv * xv * polys[2 * n + i]) % R for i in range(n)]
    q, ys = m.div_points_ints(f, zs)
    assert vals == m.encode(ys, layout) and dev.get(d_p, 32 * n) == m.encode(q, layout)
    assert o.decode_jacobian_mont_le(out.raw) == mul_ref.expected(1, p.eval_ints(q, tau), mul_ref.GEN[1])
    assert (p.eval_ints(q, tau) * m.vanishing_eval(zs, tau) + m.interpolate_eval(zs, ys, tau)) % R == p.eval_ints(f, tau)


# ---- 5. the driver -------------------------------------------------------------------------------------------------------------------
def test_stale_workspaces_and_a_second_k(msm_pkg):
    """a fresh ctx: the workspace of k = 2 regrows for k = 7 and is reused for k = 3; stale bytes change nothing"""
    n, layout = TILE * 3 + 7, m.CANON_LE
    data = m.encode(m.random_values(9, 2 * n), layout)
    c2 = msm_pkg.setup_metal_state()
    dev = Device(c2)
    try:
        def run(k):
            z = m.point_sets(layout, k, 1)[3][1]
            return (device_div(dev, data, z, layout, 2, False), device_eval(dev, data, z, layout, 2),
                    c2.fr_poly_div_points(data, z, layout, 2)[:2], c2.fr_poly_eval_points(data, z, layout, 2)[0])

        first = {k: run(k) for k in (2, 7, 3)}
        for fill in (0xFF, 0x00):
            c2.test_fill_workspaces(fill)
            for k in (3, 7, 2):
                assert run(k) == first[k], (fill, k)
        for k, got in first.items():
            exp = m.div_points(data, m.point_sets(layout, k, 1)[3][1], layout, 2)
            assert got[0] == exp and got[1] == exp[1] and got[2] == exp and got[3] == exp[1], k
    finally:
        dev.close()
        c2.close()


def test_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    n, layout = TILE + 3, m.MONT_LE
    data = m.encode(m.random_values(4, n), layout)
    z = m.encode([7, 8, 9], layout)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        d = c2.alloc(32 * n)
        c2.to_device(d, data)
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_poly_eval_points", lambda: c2.fr_poly_eval_points(d, z, layout, 1, DEVICE, n)),
                           ("msm_amd_fr_poly_eval_points", lambda: c2.fr_poly_eval_points(data, z)),
                           ("msm_amd_fr_poly_div_points", lambda: c2.fr_poly_div_points(d, z, layout, 1, DEVICE, n, d)),
                           ("msm_amd_fr_poly_div_points", lambda: c2.fr_poly_div_points(data, z))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data            # the refused calls wrote nothing
        assert c2.fr_poly_eval_points(d, z, layout, 1, DEVICE, n)[0] == m.eval_points(data, z, layout)
        assert c2.fr_poly_div_points(data, z)[:2] == m.div_points(data, z, layout)
        c2.free(d)
    finally:
        c2.close()


def test_argument_errors_and_empty_calls(cfg, msm_pkg, dev):
    L, vp = msm_pkg.lib(), ctypes.c_void_p
    bad, ok = msm_pkg.INPUT_ERROR, msm_pkg.OK
    n, k, be32 = 16, 3, msm_pkg.SCALAR_CANON_BE32
    a = m.encode(m.random_values(3, 3 * n), m.MONT_LE)
    z = m.encode([5, 6, 7], m.MONT_LE)
    z9 = m.encode(list(range(2, 11)), m.MONT_LE)
    d_a, d_out = dev.put(a + a), dev.put(b"\xA5" * len(a))
    y = ctypes.create_string_buffer(b"\xA5" * (32 * 27), 32 * 27)
    ms = ctypes.c_float(0)

    def fev(mem, layout, zz, kk, src, nn, nv, yy):
        return L.msm_amd_fr_poly_eval_points(cfg.h, mem, layout, zz, kk, vp(src) if mem == DEVICE else src, nn, nv, yy, ctypes.byref(ms))

    def fdiv(mem, layout, zz, kk, src, nn, nv, out, vals):
        return L.msm_amd_fr_poly_div_points(cfg.h, mem, layout, zz, kk, vp(src) if mem == DEVICE else src, nn, nv,
                                            vp(out) if mem == DEVICE else out, vals, ctypes.byref(ms))

    h_out = ctypes.create_string_buffer(b"\xA5" * len(a), len(a))
    for mem, src, out in ((DEVICE, d_a, d_out), (HOST, a, h_out)):
        for layout in (be32, 7):                                                  # layout
            assert fev(mem, layout, z, k, src, n, 3, y) == bad and fdiv(mem, layout, z, k, src, n, 3, out, y) == bad
        for kk in (0, 9):                                                         # k
            assert fev(mem, 0, z9, kk, src, n, 3, y) == bad and fdiv(mem, 0, z9, kk, src, n, 3, out, y) == bad
            assert b"k must be 1 .. MSM_AMD_POLY_MAX_POINTS" in L.msm_amd_last_error(cfg.h)
        assert fev(mem, 0, None, k, src, n, 3, y) == bad and fdiv(mem, 0, None, k, src, n, 3, out, y) == bad      # null z
        assert b"null z" in L.msm_amd_last_error(cfg.h)
        assert fev(mem, 0, z, k, None, n, 3, y) == bad and fdiv(mem, 0, z, k, None, n, 3, out, y) == bad          # null pointers
        assert fev(mem, 0, z, k, src, n, 3, None) == bad and fdiv(mem, 0, z, k, src, n, 3, None, y) == bad
        assert b"msm_amd_fr_poly_div_points" in L.msm_amd_last_error(cfg.h)
        assert fev(mem, 0, z, k, src, 1 << 16, 1 << 16, y) == bad and fdiv(mem, 0, z, k, src, 1 << 32, 1, out, y) == bad
    for mem in (2, -1):                                                           # mem
        assert fev(mem, 0, z, k, a, n, 3, y) == bad and fdiv(mem, 0, z, k, a, n, 3, h_out, y) == bad
        assert b"mem must be" in L.msm_amd_last_error(cfg.h)
    assert fev(DEVICE, 0, z, k, d_a + 8, n, 3, y) == bad                           # alignment
    assert fdiv(DEVICE, 0, z, k, d_a + 4, n, 3, d_out, y) == bad and fdiv(DEVICE, 0, z, k, d_a, n, 3, d_out + 8, y) == bad
    assert fdiv(DEVICE, 0, z, k, d_a, n, 3, d_a + 32, y) == bad                    # partial overlap
    assert fdiv(DEVICE, 0, z, k, d_a + 32, n, 3, d_a, y) == bad
    assert fev(DEVICE, 0, z, k, d_a, n, 3, y) == ok and ms.value >= 0
    assert L.msm_amd_fr_poly_eval_points(None, DEVICE, 0, z, k, vp(d_a), n, 3, y, None) == bad
    y = ctypes.create_string_buffer(b"\xA5" * (32 * 27), 32 * 27)
    # nothing to do: OK, nothing touched
    for nn, nv in ((0, 3), (5, 0)):
        assert fev(DEVICE, 0, z, k, None, nn, nv, y) == ok and fdiv(DEVICE, 0, z, k, None, nn, nv, None, y) == ok
        assert fev(HOST, 0, z, k, None, nn, nv, y) == ok and fdiv(HOST, 0, z, k, None, nn, nv, None, y) == ok
    assert cfg.fr_poly_eval_points(b"", z)[0] == b"" and cfg.fr_poly_div_points(b"", z)[:2] == (b"", b"")
    assert dev.get(d_out, len(a)) == b"\xA5" * len(a) and dev.get(d_a, 2 * len(a)) == a + a
    assert h_out.raw == b"\xA5" * len(a) and y.raw == b"\xA5" * (32 * 27)
    # vals_out is optional
    assert device_div(dev, a, z, m.MONT_LE, 3, False, vals=False) == (m.div_points(a, z, m.MONT_LE, 3)[0], None)


# ---- 6. guard bands: the division writes its n n_vec records, the evaluation nothing on the device ------------------------------------
@pytest.mark.parametrize("n, k", [(TILE - 1, 2), (TILE, 8), (TILE + 1, 5), (3, 8)])
def test_guard_bands(cfg, msm_pkg, n, k):
    L, n_vec = msm_pkg.lib(), 3
    layout = (n + k) & 1
    a = m.encode(m.random_values(n + k, n * n_vec), layout)
    z = m.point_sets(layout, k, n)[0][1]
    q, vals = m.div_points(a, z, layout, n_vec)

    def call(fn, mem, *args, ok=0):
        with Arena(cfg) as arena, HostArena() as host:
            return guarded(host if mem == HOST else arena, fn, cfg.h, mem, layout, *args, ok=ok, host_arena=host)

    for mem in (DEVICE, HOST):
        nv = 32 * n_vec * k
        assert call(L.msm_amd_fr_poly_eval_points, mem, z, k, In(a), n, n_vec, Out(nv, host=True), None) == [vals]
        assert call(L.msm_amd_fr_poly_div_points, mem, z, k, In(a), n, n_vec, Out(len(a)), Out(nv, host=True), None) == [q, vals]
        assert call(L.msm_amd_fr_poly_div_points, mem, z, k, In(a), n, n_vec, Out(len(a)), None, None) == [q]
        io = Out(data=a)
        assert call(L.msm_amd_fr_poly_div_points, mem, z, k, io, n, n_vec, io, Out(nv, host=True), None) == [q, vals]
        # refused calls leave the arena as it was: k out of range, an equal pair, a partial overlap
        bad = msm_pkg.INPUT_ERROR
        call(L.msm_amd_fr_poly_div_points, mem, z, 9, In(a), n, n_vec, Out(len(a)), Out(nv, host=True), None, ok=bad)
        call(L.msm_amd_fr_poly_eval_points, mem, z, 0, In(a), n, n_vec, Out(nv, host=True), None, ok=bad)
        if k >= 2:
            same = z[:32] + z[32:-32] + m.same_mod_r(z[:32])
            call(L.msm_amd_fr_poly_div_points, mem, same, k, In(a), n, n_vec, Out(len(a)), Out(nv, host=True), None, ok=bad)
        io = Out(data=a + bytes(32))
        call(L.msm_amd_fr_poly_div_points, mem, z, k, io, n, n_vec, At(io, 32), Out(nv, host=True), None, ok=bad)
