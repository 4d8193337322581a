"""The Fr vector calls on the GPU (msm_amd_fr_map*, msm_amd_fr_batch_inverse*, msm_amd_fr_prefix_product*) against the
host twins and the big-integer model of tests/fr_ref.py (tests/test_fr_host.py pins the twins to the model on the CPU).
Every comparison is of bytes: device call = host-buffer call = twin = model, unless a test says otherwise.  The scan works
on tiles of 2^T records (T = 9; the inversion on 2^8): sizes sit on both sides of a tile, MSM_AMD_FR_TILE_LOG brings
three and more levels down to a few hundred records."""
import random

import pytest

import fr_ref as m
import ntt_ref

pytestmark = pytest.mark.gpu

R = m.R
T = 9
TILE = 1 << T
INV_TILE = 1 << 8
BIG = 1 << 20


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


def operands(seed, n, layout):
    return [m.encode(m.random_values(seed + j, n), layout) for j in range(3)]


def k_record(seed, layout):
    return m.encode([random.Random(seed).randrange(1, R)], layout)


def device_map(dev, op, layout, recs, k, target=None):
    """target None: out of place into 0xFF bytes, the inputs must survive; 0 .. 2: in place on that operand"""
    n = len(recs[0]) // 32
    d = [dev.put(x) for x in recs]
    d_out = dev.put(b"\xFF" * (32 * n)) if target is None else d[target]
    ms = dev.cfg.fr_map_device(op, d[0], d[1], d[2], n, d_out, k, layout)
    assert ms >= 0
    for j in range(3):
        if j != target:
            assert dev.get(d[j], 32 * n) == recs[j], (op, j, "input changed")
    out = dev.get(d_out, 32 * n)
    dev.close()
    return out


def device_unary(dev, call, data, in_place, *args, **kw):
    d_in = dev.put(data)
    d_out = d_in if in_place else dev.put(b"\xFF" * len(data))
    ret = call(d_in, len(data) // 32 // kw.get("n_vec", 1), d_out, *args, **kw)
    if not in_place:
        assert dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, len(data))
    dev.close()
    return out, ret


# ---- 1. the map -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("op", m.OPS)
def test_map(cfg, msm_pkg, dev, op, layout):
    for n in (1, 63, 64, 65, 4097):
        recs = operands(20 * n + op, n, layout)
        k = k_record(n, layout)
        exp = m.fr_map(op, layout, *recs, k)
        assert m.first_difference(msm_pkg.host_fr_map(op, *recs, k, layout), exp) is None, n
        assert m.first_difference(device_map(dev, op, layout, recs, k), exp) is None, n
        assert m.first_difference(cfg.fr_map(op, *recs, k, layout), exp) is None, n
        if n in (65, 4097):
            for target in range(3):
                if "abc"[target] in m.READS[op]:
                    assert m.first_difference(device_map(dev, op, layout, recs, k, target), exp) is None, (n, target)
    # a == b, out of place and in place
    n = 65
    a = operands(7 + op, n, layout)[0]
    k = k_record(op, layout)
    exp = m.fr_map(op, layout, a, a, a, k)
    d_a, d_out = dev.put(a), dev.put(b"\xFF" * (32 * n))
    cfg.fr_map_device(op, d_a, d_a, d_a, n, d_out, k, layout)
    assert dev.get(d_out, 32 * n) == exp and dev.get(d_a, 32 * n) == a
    cfg.fr_map_device(op, d_a, d_a, d_a, n, d_a, k, layout)
    assert dev.get(d_a, 32 * n) == exp


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_map_unreduced_inputs(cfg, msm_pkg, dev, layout):
    a, b, c = m.raw(m.UNREDUCED), m.raw(m.UNREDUCED[::-1]), m.raw(m.UNREDUCED[2:] + m.UNREDUCED[:2])
    for op in m.OPS:
        for kw in (m.UNREDUCED[0], m.UNREDUCED[2], m.UNREDUCED[4]):
            k = m.raw([kw])
            exp = m.fr_map(op, layout, a, b, c, k)
            assert m.first_difference(device_map(dev, op, layout, [a, b, c], k), exp) is None, (op, kw)
            assert cfg.fr_map(op, a, b, c, k, layout) == exp
            assert msm_pkg.host_fr_map(op, a, b, c, k, layout) == exp
    for mode in m.MODES:
        out, _ = device_unary(dev, cfg.fr_prefix_product_device, a[32:], False, mode, layout)
        assert out == m.prefix_product(a[32:], layout, mode)
    out, (zeros, _) = device_unary(dev, cfg.fr_batch_inverse_device, a, False, layout)
    assert (out, zeros) == m.batch_inverse(a, layout)


# ---- 2. running products at the default tile ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", m.MODES)
def test_prefix_default_tile(cfg, msm_pkg, dev, mode):
    stale = m.encode(m.random_values(1, TILE + 5), m.MONT_LE)
    device_unary(dev, cfg.fr_prefix_product_device, stale, False, mode, m.MONT_LE)        # other data first: stale totals
    for n in (1, 2, TILE - 1, TILE, TILE + 1, (1 << 16) + 3):
        layout = n & 1
        data = m.encode(m.random_values(30 + n, n), layout)
        exp = m.prefix_product(data, layout, mode)
        assert msm_pkg.test_fr_plan(n, 1, T)["levels"] == (1 if n <= TILE else 2)
        assert m.first_difference(msm_pkg.host_fr_prefix_product(data, mode, layout), exp) is None, n
        out, ms = device_unary(dev, cfg.fr_prefix_product_device, data, n == TILE + 1, mode, layout)
        assert m.first_difference(out, exp) is None, n
        assert m.first_difference(cfg.fr_prefix_product(data, mode, layout), exp) is None, n


@pytest.mark.parametrize("mode", m.MODES)
def test_prefix_vectors_restart(cfg, msm_pkg, dev, mode):
    """three vectors of 2^T + 1: the tile boundaries and the vector boundaries fall apart"""
    n, n_vec = TILE + 1, 3
    vals = m.random_values(50, n * n_vec)
    data = m.encode(vals, m.MONT_LE)
    exp = m.prefix_product(data, m.MONT_LE, mode, n_vec)
    out, _ = device_unary(dev, cfg.fr_prefix_product_device, data, False, mode, m.MONT_LE, n_vec=n_vec)
    assert m.first_difference(out, exp) is None
    for v in (1, 2):   # the record behind a vector boundary knows nothing of the vector before it
        first = m.decode(out[32 * n * v:32 * n * v + 32], m.MONT_LE)[0]
        assert first == (vals[n * v] if mode == m.INCLUSIVE else 1)
    assert cfg.fr_prefix_product(data, mode, m.MONT_LE, n_vec) == exp
    assert msm_pkg.host_fr_prefix_product(data, mode, m.MONT_LE, n_vec) == exp
    out, _ = device_unary(dev, cfg.fr_prefix_product_device, data, True, mode, m.MONT_LE, n_vec=n_vec)
    assert out == exp


# ---- 3. small tiles: three and more levels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_log", [2, 3])
def test_small_tiles(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_FR_TILE_LOG (read at msm_amd_init) lowers the tile to 4 or 8 records: up to five levels on at most 513"""
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", str(tile_log))
    c2 = msm_pkg.setup_metal_state()
    tile = 1 << tile_log
    try:
        assert msm_pkg.test_fr_plan(70, 1, tile_log)["levels"] >= 3
        assert msm_pkg.test_fr_plan(513, 2, tile_log)["levels"] == (5 if tile_log == 2 else 4)
        d_in, d_out = c2.alloc(32 * 513 * 2), c2.alloc(32 * 513 * 2)
        for n in list(range(1, 71)) + [257, 513]:
            for n_vec in (1, 2):
                layout, mode = n & 1, (n >> 1) & 1
                data = m.encode(m.random_values(1000 * n_vec + n, n * n_vec), layout)
                for md in (mode, 1 - mode) if n in (7, 70, 257, 513) else (mode,):
                    exp = m.prefix_product(data, layout, md, n_vec)
                    c2.to_device(d_in, data)
                    c2.to_device(d_out, b"\xFF" * len(data))
                    c2.fr_prefix_product_device(d_in, n, d_out, md, layout, n_vec)
                    assert m.first_difference(c2.to_host(d_out, len(data)), exp) is None, (n, n_vec, md)
                    assert c2.to_host(d_in, len(data)) == data
                    assert c2.fr_prefix_product(data, md, layout, n_vec) == exp, (n, n_vec, md)
            # the inversion: zeros on the first and the last record of a tile, and a whole tile of them
            vals = m.random_values(2000 + n, n)
            zeros = {i for i in (0, tile - 1, tile, 2 * tile - 1, n - 1) if i < n} if n % 3 else set()
            if n >= 4 * tile and n % 2:
                zeros |= set(range(2 * tile, 3 * tile))
            for i in zeros:
                vals[i] = 0
            layout = (n >> 1) & 1
            data = m.encode(vals, layout)
            exp = m.batch_inverse(data, layout)
            c2.to_device(d_in, data)
            c2.to_device(d_out, b"\xFF" * len(data))
            n_zero, _ = c2.fr_batch_inverse_device(d_in, n, d_out, layout)
            assert m.first_difference(c2.to_host(d_out, len(data)), exp[0]) is None, n
            assert n_zero == exp[1] == len(zeros), n
            assert c2.fr_batch_inverse(data, layout) == exp, n
        c2.free(d_in)
        c2.free(d_out)
    finally:
        c2.close()


# ---- 4. the inversion at the default tile -----------------------------------------------------------------------------------------
def test_inverse(cfg, msm_pkg, dev):
    for n in (1, 2, INV_TILE - 1, INV_TILE + 1, TILE - 1, TILE + 1, (1 << 16) + 3):
        for pattern in ("none", "one", "all"):
            layout = (n + len(pattern)) & 1
            vals = m.random_values(60 + n, n)
            if pattern == "one":
                vals[n // 2] = 0
            if pattern == "all":
                vals = [0] * n
            data = m.encode(vals, layout)
            exp = m.batch_inverse(data, layout)
            assert msm_pkg.host_fr_batch_inverse(data, layout) == exp, (n, pattern)
            out, (zeros, ms) = device_unary(dev, cfg.fr_batch_inverse_device, data, pattern == "one", layout)
            assert m.first_difference(out, exp[0]) is None, (n, pattern)
            assert zeros == exp[1] == {"none": 0, "one": 1, "all": n}[pattern]
            assert cfg.fr_batch_inverse(data, layout) == exp, (n, pattern)
        # the call after an all-zero one starts clean
        data = m.encode(m.random_values(61 + n, min(n, TILE + 1)), m.MONT_LE)
        assert cfg.fr_batch_inverse(data, m.MONT_LE) == m.batch_inverse(data, m.MONT_LE)


# ---- 5. a large size without a large model ------------------------------------------------------------------------------------------
def test_large_prefix_of_a_constant(cfg, dev):
    g = 0x1234567890ABCDEF1234567890ABCDEF
    data = m.encode([g], m.MONT_LE) * BIG
    d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
    assert cfg.fr_prefix_product_device(d_in, BIG, d_out) > 0
    out = dev.get(d_out, len(data))
    for i in sorted(set(random.Random(5).sample(range(BIG), 2000)) | {0, TILE - 1, TILE, BIG // 2, BIG - 1}):
        assert out[32 * i:32 * i + 32] == m.encode([pow(g, i + 1, R)], m.MONT_LE), i


def test_large_inverse_against_the_twin(cfg, msm_pkg, dev):
    raw = bytearray(random.Random(20).randbytes(32 * BIG))
    raw[31::32] = bytes(b & 0x1F for b in raw[31::32])    # every record < 2^253 < r: reduced MONT_LE records
    data = bytes(raw)
    exp, exp_zero = msm_pkg.host_fr_batch_inverse(data, m.MONT_LE)
    d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
    zeros, ms = cfg.fr_batch_inverse_device(d_in, BIG, d_out)
    out = dev.get(d_out, len(data))
    assert m.first_difference(out, exp) is None
    assert zeros == exp_zero == 0 and ms > 0
    for i in random.Random(6).sample(range(BIG), 1000):
        x, y = m.decode(data[32 * i:32 * i + 32], m.MONT_LE)[0], m.decode(out[32 * i:32 * i + 32], m.MONT_LE)[0]
        assert x * y % R == 1, i


# ---- 6. Groth16's quotient, on the device from the first call to the last -----------------------------------------------------------
@pytest.mark.parametrize("log_n", [6, 10])
def test_groth16_quotient_recipe(cfg, dev, log_n):
    n, layout, g = 1 << log_n, m.MONT_LE, 7
    rng = random.Random(log_n)
    A, B = m.random_values(600 + log_n, n), m.random_values(700 + log_n, n)
    C = [x * y % R for x, y in zip(A, B)]                     # c = a b on H
    d = [dev.put(m.encode(v, layout)) for v in (A, B, C)]
    shift = ntt_ref.shift_record(g, layout)
    k = m.encode([pow(pow(g, n, R) - 1, -1, R)], layout)      # x^n - 1 = g^n - 1 on the coset g H
    dom = cfg.ntt_domain(ntt_ref.ARK, log_n)
    try:
        for p in d:
            cfg.ntt_device(dom, p, p, ntt_ref.INVERSE, layout)                    # coefficients
        for p in d:
            cfg.ntt_device(dom, p, p, ntt_ref.FORWARD, layout, shift)             # evaluations on g H
        cfg.fr_map_device(m.MULSUB_SCALE, d[0], d[1], d[2], n, d[0], k, layout)   # h = (a b - c) / (x^n - 1) there
        cfg.ntt_device(dom, d[0], d[0], ntt_ref.INVERSE, layout, shift)           # the coefficients of h
        h = m.decode(dev.get(d[0], 32 * n), layout)
    finally:
        dom.free()
    a, b, c = (ntt_ref.transform(v, ntt_ref.ARK, log_n, ntt_ref.INVERSE) for v in (A, B, C))

    def at(poly, x):
        acc = 0
        for coeff in reversed(poly):
            acc = (acc * x + coeff) % R
        return acc

    assert any(h)
    for _ in range(2):
        x = rng.randrange(R)
        assert (at(a, x) * at(b, x) - at(c, x)) % R == at(h, x) * (pow(x, n, R) - 1) % R


# ---- 7. the grand product of a permutation argument ---------------------------------------------------------------------------------
def test_grand_product_recipe(cfg, dev):
    n, layout = 1000, m.CANON_LE
    num = [v or 1 for v in m.random_values(80, n)]
    den = num[:]
    random.Random(81).shuffle(den)
    d_num, d_den, d_z = dev.put(m.encode(num, layout)), dev.put(m.encode(den, layout)), dev.put(b"\xFF" * (32 * n))
    zeros, _ = cfg.fr_batch_inverse_device(d_den, n, d_den, layout)
    assert zeros == 0
    cfg.fr_map_device(m.MUL, d_num, d_den, None, n, d_den, None, layout)             # q = num / den
    cfg.fr_prefix_product_device(d_den, n, d_z, m.EXCLUSIVE, layout)
    z, q = m.decode(dev.get(d_z, 32 * n), layout), m.decode(dev.get(d_den, 32 * n), layout)
    exp, run = [], 1
    for x, y in zip(num, den):
        exp.append(run)
        run = run * x * pow(y, -1, R) % R
    assert run == 1
    assert z == exp and z[0] == 1 and z[n - 1] * q[n - 1] % R == 1
    assert z[n - 1] * num[n - 1] * pow(den[n - 1], -1, R) % R == 1


# ---- 8. the driver -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(cfg, msm_pkg, dev):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    n = 16
    a, b, c = operands(3, n, m.MONT_LE)
    k = k_record(3, m.MONT_LE)
    d_a, d_b, d_c = dev.put(a + a), dev.put(b), dev.put(c)
    d_out = dev.put(b"\xA5" * (32 * n))
    fmap, finv, fpre = cfg.fr_map_device, cfg.fr_batch_inverse_device, cfg.fr_prefix_product_device
    input_error(fmap, 6, d_a, d_b, d_c, n, d_out, k)                                   # op
    input_error(fmap, m.ADD, d_a, d_b, d_c, n, d_out, k, msm_pkg.SCALAR_CANON_BE32)    # layout
    input_error(fmap, m.ADD, None, d_b, d_c, n, d_out, k)                              # a null operand that is read
    input_error(fmap, m.MULSUB_SCALE, d_a, d_b, None, n, d_out, k)
    input_error(fmap, m.AXPY, d_a, d_b, None, n, d_out, None)                          # k is read
    input_error(fmap, m.ADD, d_a, d_b, None, n, None)
    input_error(fmap, m.ADD, d_a + 8, d_b, None, n, d_out)                             # alignment
    input_error(fmap, m.ADD, d_a, d_b + 4, None, n, d_out)
    input_error(fmap, m.ADD, d_a, d_b, None, n, d_out + 8)
    input_error(fmap, m.ADD, d_a, d_b, None, n, d_a + 32)                              # partial overlap
    input_error(fmap, m.ADD, d_a + 32, d_b, None, n, d_a)
    input_error(fmap, m.ADD, d_b, d_a + 32 * n, None, n, d_a + 32)
    input_error(fmap, m.ADD, d_a, d_b, None, 1 << 32, d_out)
    input_error(finv, d_a, n, d_out, msm_pkg.SCALAR_CANON_BE32)
    input_error(finv, None, n, d_out)
    input_error(finv, d_a, n, None)
    input_error(finv, d_a + 16, n, d_out + 8)
    input_error(finv, d_a, n, d_a + 32)
    input_error(finv, d_a, 1 << 32, d_out)
    input_error(fpre, d_a, n, d_out, 2)                                                # mode
    input_error(fpre, d_a, n, d_out, 0, msm_pkg.SCALAR_CANON_BE32)
    input_error(fpre, None, n, d_out)
    input_error(fpre, d_a, n, d_out + 8)
    input_error(fpre, d_a, n, d_a + 32)
    input_error(fpre, d_a + 32, n, d_a)
    input_error(fpre, d_a, 1 << 16, d_out, 0, 0, 1 << 16)                              # n n_vec = 2^32
    input_error(cfg.fr_map, m.ADD, a, None)
    input_error(cfg.fr_map, 9, a, b)
    input_error(cfg.fr_batch_inverse, a, msm_pkg.SCALAR_CANON_BE32)
    input_error(cfg.fr_prefix_product, a, 5)
    assert dev.get(d_out, 32 * n) == b"\xA5" * (32 * n) and dev.get(d_a, 64 * n) == a + a
    # nothing to do: OK, nothing touched
    fmap(m.ADD, None, None, None, 0, None)
    assert finv(None, 0, None)[0] == 0
    fpre(None, 0, None, 0, 0, 3)
    fpre(None, 5, None, 0, 0, 0)
    assert cfg.fr_map(m.ADD, b"", b"") == b"" and cfg.fr_batch_inverse(b"") == (b"", 0) and cfg.fr_prefix_product(b"") == b""
    assert dev.get(d_out, 32 * n) == b"\xA5" * (32 * n)
    # operands the op does not read are ignored, whatever they are
    fmap(m.SCALE, d_a, d_a + 8, d_out + 4, n, d_out, k)
    assert dev.get(d_out, 32 * n) == m.fr_map(m.SCALE, m.MONT_LE, a, k=k)


def test_stale_workspaces_change_nothing(cfg, msm_pkg, dev):
    n = TILE + 7
    vals = m.random_values(9, n)
    vals[5] = 0
    data = m.encode(vals, m.CANON_LE)
    first_inv = device_unary(dev, cfg.fr_batch_inverse_device, data, False, m.CANON_LE)
    first_pre = device_unary(dev, cfg.fr_prefix_product_device, data, False, m.EXCLUSIVE, m.CANON_LE)
    host = cfg.fr_batch_inverse(data, m.CANON_LE), cfg.fr_map(m.MUL, data, data, None, None, m.CANON_LE)
    cfg.test_fill_workspaces(0xFF)
    out, (zeros, _) = device_unary(dev, cfg.fr_batch_inverse_device, data, False, m.CANON_LE)
    assert (out, zeros) == (first_inv[0], 1) == m.batch_inverse(data, m.CANON_LE)
    assert device_unary(dev, cfg.fr_prefix_product_device, data, False, m.EXCLUSIVE, m.CANON_LE)[0] == first_pre[0]
    assert first_pre[0] == m.prefix_product(data, m.CANON_LE, m.EXCLUSIVE)
    assert (cfg.fr_batch_inverse(data, m.CANON_LE), cfg.fr_map(m.MUL, data, data, None, None, m.CANON_LE)) == host


def test_fr_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    n = TILE + 3
    data = m.encode(m.random_values(4, n), m.MONT_LE)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        d = c2.alloc(32 * n)
        c2.to_device(d, data)
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_map_device", lambda: c2.fr_map_device(m.MUL, d, d, None, n, d)),
                           ("msm_amd_fr_map", lambda: c2.fr_map(m.MUL, data, data)),
                           ("msm_amd_fr_batch_inverse_device", lambda: c2.fr_batch_inverse_device(d, n, d)),
                           ("msm_amd_fr_batch_inverse", lambda: c2.fr_batch_inverse(data)),
                           ("msm_amd_fr_prefix_product_device", lambda: c2.fr_prefix_product_device(d, n, d)),
                           ("msm_amd_fr_prefix_product", lambda: c2.fr_prefix_product(data))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data            # the refused calls wrote nothing
        c2.fr_batch_inverse_device(d, n, d)
        assert c2.to_host(d, len(data)) == m.batch_inverse(data, m.MONT_LE)[0]
        assert c2.fr_prefix_product(data) == m.prefix_product(data, m.MONT_LE, m.INCLUSIVE)
        c2.free(d)
    finally:
        c2.close()
