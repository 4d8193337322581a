"""The polynomial calls on the GPU (msm_amd_fr_poly_eval*, msm_amd_fr_poly_div_linear*, msm_amd_fr_lincomb*) against the
host twins and the big-integer model of tests/poly_ref.py (tests/test_poly_host.py pins the twins to the model on the CPU).
Every comparison is of bytes: device call = host-buffer call = twin = model.  The kernels work on the tiles and levels of
the prefix products (2^T records, T = 9): sizes sit on both sides of a tile and of a level, MSM_AMD_FR_TILE_LOG brings five
levels down to a few hundred records."""
import ctypes
import random

import pytest

import mul_ref
import poly_ref as m
from oracle import bn254_ref as o

pytestmark = pytest.mark.gpu

R = m.R
T = 9
TILE = 1 << T
BIG = 1 << 20
_POOL = {}


def pool(n):
    """the first n of 5 (2^16 + 3) random values, drawn once"""
    if not _POOL:
        _POOL["v"] = m.random_values(2024, 5 * ((1 << 16) + 3))
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


def device_div(dev, data, z, layout, n_vec, in_place):
    """the division on fresh buffers: out of place into 0xFF bytes, and the input must survive"""
    n = len(data) // 32 // n_vec
    d_in = dev.put(data)
    d_out = d_in if in_place else dev.put(b"\xFF" * len(data))
    rem, ms = dev.cfg.fr_poly_div_linear_device(d_in, n, d_out, z, layout, n_vec)
    assert ms >= 0
    if not in_place:
        assert dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, len(data))
    dev.close()
    return out, rem


def device_eval(dev, data, z, layout, n_vec):
    d_in = dev.put(data)
    y, ms = dev.cfg.fr_poly_eval_device(d_in, len(data) // 32 // n_vec, z, layout, n_vec)
    assert ms >= 0 and dev.get(d_in, len(data)) == data
    dev.close()
    return y


def device_lincomb(dev, data, k, layout, n_vec, in_place):
    n = len(data) // 32 // n_vec
    d_a = dev.put(data)
    d_out = d_a if in_place else dev.put(b"\xFF" * (32 * n))
    assert dev.cfg.fr_lincomb_device(d_a, n, d_out, k, layout, n_vec) >= 0
    rest = dev.get(d_a, len(data))
    out = dev.get(d_out, 32 * n)
    assert rest[32 * n if in_place else 0:] == data[32 * n if in_place else 0:], "input changed"
    dev.close()
    return out


def check_poly(cfg, msm_pkg, dev, data, z, layout, n_vec, tag, in_place=(False,)):
    """evaluation and division: device call = host-buffer call = twin = model"""
    exp_q, exp_rem = m.div_linear(data, z, layout, n_vec)
    assert exp_rem == m.poly_eval(data, z, layout, n_vec), tag
    q, rem = msm_pkg.host_fr_poly_div_linear(data, z, layout, n_vec)
    assert m.first_difference(q, exp_q) is None and rem == exp_rem, tag
    assert msm_pkg.host_fr_poly_eval(data, z, layout, n_vec) == exp_rem, tag
    for ip in in_place:
        q, rem = device_div(dev, data, z, layout, n_vec, ip)
        assert m.first_difference(q, exp_q) is None, (tag, ip)
        assert rem == exp_rem, (tag, ip)
    assert device_eval(dev, data, z, layout, n_vec) == exp_rem, tag
    assert cfg.fr_poly_div_linear(data, z, layout, n_vec) == (exp_q, exp_rem), tag
    assert cfg.fr_poly_eval(data, z, layout, n_vec) == exp_rem, tag


# ---- 1. small tiles: up to five levels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_log", [2, 3])
def test_small_tiles(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_FR_TILE_LOG (read at msm_amd_init) lowers the tile to 4 or 8 records"""
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", str(tile_log))
    c2 = msm_pkg.setup_metal_state()
    dev = Device(c2)
    try:
        assert msm_pkg.test_fr_plan(70, 1, tile_log)["levels"] >= 3
        assert msm_pkg.test_fr_plan(513, 2, tile_log)["levels"] == (5 if tile_log == 2 else 4)
        for n in list(range(1, 71)) + [257, 513]:
            layout = n & 1
            points = m.special_points(layout)
            for n_vec in (1, 2):
                data = m.encode(m.random_values(1000 * n_vec + n, n * n_vec), layout)
                for name, z in (points[6], points[(n + n_vec) % 6]):
                    check_poly(c2, msm_pkg, dev, data, z, layout, n_vec, (n, n_vec, name), (bool((n + n_vec) & 1),))
            data = m.encode(m.random_values(3000 + n, n * 3), layout)
            k = points[6][1] if n % 4 else points[n % 6][1]
            exp = m.lincomb(data, k, layout, 3)
            assert msm_pkg.host_fr_lincomb(data, k, layout, 3) == exp, n
            assert device_lincomb(dev, data, k, layout, 3, bool(n & 2)) == exp, n
            assert c2.fr_lincomb(data, k, layout, 3) == exp, n
    finally:
        dev.close()
        c2.close()


# ---- 2. the default tile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 1025, 1 << 18, (1 << 18) + 1])
def test_default_tile(cfg, msm_pkg, dev, n):
    """2^18 + 1 is the first size of three levels, and its top tile holds two records"""
    levels = msm_pkg.test_fr_plan(n, 1, T)["levels"]
    assert levels == (1 if n <= TILE else 2 if n <= TILE * TILE else 3)
    layout = n & 1
    points = m.special_points(layout)
    data = m.encode(pool(n), layout)
    names = (6,) if n > 1025 else (6, 0, 1, 2, 3, 4, 5)
    for j in names:
        name, z = points[j]
        check_poly(cfg, msm_pkg, dev, data, z, layout, 1, (n, name), (False, True) if j == 6 else (False,))
    if n <= 1025:   # unreduced words
        words = [((3 * i + 1) * R // 7 + i) % (1 << 256) for i in range(n)]
        check_poly(cfg, msm_pkg, dev, m.raw(words), points[6][1], layout, 1, (n, "unreduced"))


@pytest.mark.parametrize("n", [513, 1025])
def test_three_vectors(cfg, msm_pkg, dev, n):
    """the tile boundaries and the vector boundaries fall apart; in place, and into 0xFF-filled memory with the inputs intact"""
    for layout in m.LAYOUTS:
        data = m.encode(m.random_values(50 + n, 3 * n), layout)
        z = m.special_points(layout)[6][1]
        check_poly(cfg, msm_pkg, dev, data, z, layout, 3, (n, layout), (False, True))
        alone = [msm_pkg.host_fr_poly_div_linear(data[32 * n * v:32 * n * (v + 1)], z, layout) for v in range(3)]
        q, rem = device_div(dev, data, z, layout, 3, False)
        assert q == b"".join(a[0] for a in alone) and rem == b"".join(a[1] for a in alone)     # the vectors restart
    d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
    assert cfg.fr_poly_div_linear_device(d_in, n, d_out, z, layout, 3, rem=False)[0] is None    # rem_out is optional
    assert dev.get(d_out, len(data)) == m.div_linear(data, z, layout, 3)[0]


# ---- 3. the fold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vec", [1, 2, 5])
def test_lincomb(cfg, msm_pkg, dev, n_vec):
    for n in (1, 255, 256, 257, (1 << 16) + 3):
        layout = (n + n_vec) & 1
        points = m.special_points(layout)
        data = m.encode(pool(n * n_vec), layout)
        for name, k in (points[6], points[n % 6]):
            exp = m.lincomb(data, k, layout, n_vec)
            assert msm_pkg.host_fr_lincomb(data, k, layout, n_vec) == exp, (n, name)
            assert m.first_difference(device_lincomb(dev, data, k, layout, n_vec, False), exp) is None, (n, name)
            assert m.first_difference(device_lincomb(dev, data, k, layout, n_vec, True), exp) is None, (n, name)
            assert cfg.fr_lincomb(data, k, layout, n_vec) == exp, (n, name)
    words = m.raw([((5 * i + 2) * R // 3 + i) % (1 << 256) for i in range(257 * n_vec)])
    assert device_lincomb(dev, words, points[6][1], layout, n_vec, False) == m.lincomb(words, points[6][1], layout, n_vec)


# ---- 4. a large size without a large model -------------------------------------------------------------------------------------
def test_large_division_of_all_ones(cfg, msm_pkg, dev):
    n, layout, zv = BIG, m.MONT_LE, 5
    z = m.encode([zv], layout)
    data = m.encode([1], layout) * n
    exp_q, exp_rem = msm_pkg.host_fr_poly_div_linear(data, z, layout, 1, 16)
    d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
    rem, ms = cfg.fr_poly_div_linear_device(d_in, n, d_out, z, layout)
    out = dev.get(d_out, len(data))
    assert ms > 0 and m.first_difference(out, exp_q) is None and rem == exp_rem
    y, ms = cfg.fr_poly_eval_device(d_in, n, z, layout)
    assert ms > 0 and y == rem == msm_pkg.host_fr_poly_eval(data, z, layout, 1, 16)
    inv = pow(zv - 1, -1, R)

    def s(i):   # sum_{j >= i} z^(j - i) = (z^(n - i) - 1) / (z - 1)
        return (pow(zv, n - i, R) - 1) * inv % R

    assert rem == m.encode([s(0)], layout)
    fixed = [0, 1, 63, 64, TILE - 1, TILE, TILE * TILE - 1, TILE * TILE, n // 2, n - TILE - 1, n - TILE, n - 3, n - 2, n - 1]
    fixed += random.Random(5).sample(range(n), 64 - len(fixed))
    edges = {e for b in range(1, n // TILE) for e in (b * TILE - 1, b * TILE)}              # every tile edge of the first level
    for i in sorted(set(fixed) | edges):
        assert out[32 * i:32 * i + 32] == m.encode([s(i + 1)], layout), i
    assert out[32 * (n - 1):] == bytes(32)


# ---- 5. open at z, on the device from the first call to the last -------------------------------------------------------------------
def test_opening_recipe(cfg, msm_pkg, dev):
    """f = p_0 + k p_1 + k^2 p_2, q = (f - f(z)) / (X - z) in place, the commitment [q(tau)]G by the MSM on the same pointer"""
    n, layout = 1027, m.MONT_LE
    rng = random.Random(31)
    tau, zv, kv = rng.randrange(2, R), rng.randrange(R), rng.randrange(R)
    psize = msm_pkg.decompressed_bytes(msm_pkg.POINT_PREPARED, False)
    powers = [pow(tau, i, R) for i in range(n)]
    d_tau = dev.put(mul_ref.scalars_bytes(powers, 0))
    d_gen = dev.put(mul_ref.base_record(1, 0, mul_ref.GEN[1]))
    d_bases = dev.put(bytes(n * psize))
    cfg.mul_points_device(d_tau, d_gen, n, d_bases, msm_pkg.MUL_BASE_ONE, 0, 0, msm_pkg.POINT_PREPARED)     # [tau^i]G
    polys = m.random_values(32, 3 * n)
    data = m.encode(polys, layout)
    z, k = m.encode([zv], layout), m.encode([kv], layout)
    d_p = dev.put(data)
    cfg.fr_lincomb_device(d_p, n, d_p, k, layout, 3)
    rem, _ = cfg.fr_poly_div_linear_device(d_p, n, d_p, z, layout)
    out = ctypes.create_string_buffer(96)
    vp = ctypes.c_void_p
    assert msm_pkg.lib().msm_amd_msm_device(cfg.h, layout, msm_pkg.POINT_PREPARED, vp(d_p), vp(d_bases), n, out) == msm_pkg.OK
    f = [(polys[i] + kv * polys[n + i] + kv * kv * polys[2 * n + i]) % R for i in range(n)]
    q, y = m.div_linear_ints(f, zv)
    assert rem == m.encode([y], layout) and y == m.eval_ints(f, zv)
    assert dev.get(d_p, 32 * n) == m.encode(q, layout)
    assert o.decode_jacobian_mont_le(out.raw) == mul_ref.expected(1, m.eval_ints(q, tau), mul_ref.GEN[1])
    assert (m.eval_ints(q, tau) * (tau - zv) + y) % R == m.eval_ints(f, tau)


# ---- 6. the driver -------------------------------------------------------------------------------------------------------------------
def test_stale_workspaces_change_nothing(cfg, msm_pkg, dev):
    n, layout = TILE * 3 + 7, m.CANON_LE
    data = m.encode(m.random_values(9, 2 * n), layout)
    z = m.special_points(layout)[6][1]

    def run():
        return (device_div(dev, data, z, layout, 2, False), device_eval(dev, data, z, layout, 2),
                device_lincomb(dev, data, z, layout, 2, False), cfg.fr_poly_div_linear(data, z, layout, 2),
                cfg.fr_poly_eval(data, z, layout, 2), cfg.fr_lincomb(data, z, layout, 2))

    first = run()
    cfg.test_fill_workspaces(0xFF)
    assert run() == first
    cfg.test_fill_workspaces(0x00)
    assert run() == first
    assert first[0] == m.div_linear(data, z, layout, 2) and first[1] == m.poly_eval(data, z, layout, 2)
    assert first[2] == m.lincomb(data, z, layout, 2)


def test_poly_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    n, layout = TILE + 3, m.MONT_LE
    data = m.encode(m.random_values(4, n), layout)
    z = m.encode([7], layout)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        d = c2.alloc(32 * n)
        c2.to_device(d, data)
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_poly_eval_device", lambda: c2.fr_poly_eval_device(d, n, z)),
                           ("msm_amd_fr_poly_eval", lambda: c2.fr_poly_eval(data, z)),
                           ("msm_amd_fr_poly_div_linear_device", lambda: c2.fr_poly_div_linear_device(d, n, d, z)),
                           ("msm_amd_fr_poly_div_linear", lambda: c2.fr_poly_div_linear(data, z)),
                           ("msm_amd_fr_lincomb_device", lambda: c2.fr_lincomb_device(d, n, d, z)),
                           ("msm_amd_fr_lincomb", lambda: c2.fr_lincomb(data, z))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data            # the refused calls wrote nothing
        assert c2.fr_poly_eval_device(d, n, z)[0] == m.poly_eval(data, z, layout)
        assert c2.fr_poly_div_linear(data, z) == m.div_linear(data, z, layout)
        c2.free(d)
    finally:
        c2.close()


def test_argument_errors_and_empty_calls(cfg, msm_pkg, dev):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    n, be32 = 16, msm_pkg.SCALAR_CANON_BE32
    a = m.encode(m.random_values(3, 3 * n), m.MONT_LE)
    z = m.encode([5], m.MONT_LE)
    d_a, d_out = dev.put(a + a), dev.put(b"\xA5" * len(a))
    fev, fdiv, flc = cfg.fr_poly_eval_device, cfg.fr_poly_div_linear_device, cfg.fr_lincomb_device
    input_error(fev, d_a, n, z, be32, 3)                                  # layout
    input_error(fdiv, d_a, n, d_out, z, be32, 3)
    input_error(flc, d_a, n, d_out, z, be32, 3)
    input_error(fev, d_a, n, z, 7, 3)
    input_error(fev, None, n, z, 0, 3)                                    # null pointers
    input_error(fev, d_a, n, None, 0, 3)
    input_error(fdiv, None, n, d_out, z, 0, 3)
    input_error(fdiv, d_a, n, None, z, 0, 3)
    input_error(fdiv, d_a, n, d_out, None, 0, 3)
    input_error(flc, None, n, d_out, z, 0, 3)
    input_error(flc, d_a, n, None, z, 0, 3)
    input_error(flc, d_a, n, d_out, None, 0, 3)
    input_error(fev, d_a + 8, n, z, 0, 3)                                 # alignment
    input_error(fdiv, d_a + 4, n, d_out, z, 0, 3)
    input_error(fdiv, d_a, n, d_out + 8, z, 0, 3)
    input_error(flc, d_a + 8, n, d_out, z, 0, 3)
    input_error(flc, d_a, n, d_out + 4, z, 0, 3)
    input_error(fdiv, d_a, n, d_a + 32, z, 0, 3)                          # partial overlap
    input_error(fdiv, d_a + 32, n, d_a, z, 0, 3)
    input_error(flc, d_a, n, d_a + 32, z, 0, 3)
    input_error(flc, d_a, n, d_a + 32 * n, z, 0, 3)                       # the second vector is not a place for the result
    input_error(flc, d_a + 32, n, d_a, z, 0, 3)
    input_error(fev, d_a, 1 << 16, z, 0, 1 << 16)                         # n n_vec = 2^32
    input_error(fdiv, d_a, 1 << 32, d_out, z)
    input_error(flc, d_a, 1 << 16, d_out, z, 0, 1 << 16)
    input_error(cfg.fr_poly_eval, a, z, be32, 3)
    input_error(cfg.fr_poly_div_linear, a, None, 0, 3)
    input_error(cfg.fr_lincomb, a, z, be32, 3)
    L, vp = msm_pkg.lib(), ctypes.c_void_p
    assert L.msm_amd_fr_poly_eval_device(cfg.h, 0, z, vp(d_a), n, 3, None, None) == msm_pkg.INPUT_ERROR     # y_out is required
    assert b"msm_amd_fr_poly_eval_device" in L.msm_amd_last_error(cfg.h)
    assert dev.get(d_out, len(a)) == b"\xA5" * len(a) and dev.get(d_a, 2 * len(a)) == a + a
    # nothing to do: OK, nothing touched
    assert fev(None, 0, None, 0, 3)[0] == b"" and fev(None, 5, None, 0, 0)[0] == b""
    assert fdiv(None, 0, None, None, 0, 3)[0] == b"" and fdiv(None, 5, None, None, 0, 0)[0] == b""
    flc(None, 0, None, None, 0, 3)
    flc(None, 5, None, None, 0, 0)
    assert cfg.fr_poly_eval(b"", z) == b"" and cfg.fr_poly_div_linear(b"", z) == (b"", b"") and cfg.fr_lincomb(b"", z) == b""
    assert dev.get(d_out, len(a)) == b"\xA5" * len(a)
    # right behind a is disjoint from a
    flc(d_a, n, d_a + 32 * n * 3, z, 0, 3)
    assert dev.get(d_a + 32 * n * 3, 32 * n) == m.lincomb(a, z, m.MONT_LE, 3)
