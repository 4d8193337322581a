"""The pass geometry of the transform on the GPU.  ntt_pass_kernel has no second implementation of its gather, its
two-levels-per-step butterflies, its LDS layout and its stepping of the powers of the shift: the host twin runs the
network one level at a time over a flat array.  So this file runs every kind of pass the plan can produce (tests/
ntt_shapes.py; tests/test_ntt_plan_host.py accounts for them): the two-pass sizes 2^14 .. 2^20 of the default tile, tiles
of 2^4 .. 2^9 elements with one, two and three passes, the state after each pass (msm_amd_test_ntt_passes), the twiddle
table itself, unreduced records and shifts, and batches that end inside a workgroup.  References: the integer model of
tests/ntt_ref.py up to 2^13; above that the host twin (pinned to the model on the CPU by tests/test_ntt_host.py and
tests/test_ntt_plan_host.py) together with the closed form for sparse inputs, which shares no code with either.  Every
comparison is of bytes."""
import functools
import random

import pytest

import fr_ref
import ntt_ref as m
import ntt_shapes as shapes
from test_gpu_ntt import device_ntt, first_difference, on_device

pytestmark = pytest.mark.gpu

R = m.R
MODEL_MAX_LOG = 13                                   # the model up to here, the twin above
LOW5 = bytes(b & 0x1F for b in range(256))


def dense_records(seed, count):
    """random records < 2^253 < r: reduced in either layout"""
    raw = bytearray(random.Random(seed).randbytes(32 * count))
    raw[31::32] = raw[31::32].translate(LOW5)
    return bytes(raw)


def values_of(data, layout):
    """the residues raw records stand for: any 256-bit value is read mod r, a MONT_LE record x as x 2^-256"""
    return [v % R for v in m.decode(data, layout)]


@functools.lru_cache(maxsize=None)
def model_case(seed, log_n, n_vec, direction, layout, g):
    """(input records, expected records) from the integer model; shared by every tile size"""
    n = 1 << log_n
    a = m.random_vector(seed, n_vec * n)
    exp = [x for v in range(n_vec) for x in m.transform(a[v * n:(v + 1) * n], m.H2C, log_n, direction, g or 1)]
    return m.encode(a, layout), m.encode(exp, layout)


_twin_cache = {}


def twin_case(msm_pkg, seed, log_n, n_vec, direction, layout, g):
    """(input records, expected records) from the host twin; kept for the other tile sizes while small"""
    key = (seed, log_n, n_vec, direction, layout, g)
    if key in _twin_cache:
        return _twin_cache[key]
    data = dense_records(seed, n_vec << log_n)
    case = data, msm_pkg.host_ntt(data, m.H2C, log_n, direction, layout, m.shift_record(g, layout), n_vec)
    if log_n <= 16:
        _twin_cache[key] = case
    return case


def sparse_check(c, dom, root, log_n, n_vec, g, seed):
    """FORWARD of 3 or 4 terms per vector against the closed form at 1024 sampled outputs: no shared body can hide"""
    n = 1 << log_n
    rng = random.Random(seed)
    data = bytearray(32 * n_vec * n)
    terms = []
    for v in range(n_vec):
        ts = [(1, 3), (n // 2 + 3, R - 5), (n - 1, rng.randrange(R))] + ([(rng.randrange(n), rng.randrange(R))] if (v + log_n) & 1 else [])
        ts = list(dict(ts).items())
        for i, coeff in ts:
            data[32 * (v * n + i):32 * (v * n + i) + 32] = m.encode([coeff], m.CANON_LE)
        terms.append(ts)
    out = c.ntt(dom, bytes(data), m.FORWARD, m.CANON_LE, m.shift_record(g, m.CANON_LE), n_vec)
    per_vec = 1024 // n_vec
    for v in range(n_vec):
        ks = sorted(set(rng.sample(range(n), min(n, per_vec))) | {0, n // 2, n - 1})
        for k in ks:
            got = out[32 * (v * n + k):32 * (v * n + k) + 32]
            assert got == m.encode([m.sparse_forward(terms[v], root, log_n, k, g)], m.CANON_LE), (log_n, v, k)


# ---- 1. the two-pass sizes of the default tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [log_n for _, log_n in shapes.GEOMETRY_DEFAULT])
def test_two_pass_sizes(cfg, msm_pkg, log_n):
    n = 1 << log_n
    root = log_n & 1
    g = random.Random(log_n).randrange(2, R)
    data = dense_records(1400 + log_n, n)
    dom = cfg.ntt_domain(root, log_n)
    d_in, d_out = on_device(cfg, data), cfg.alloc(32 * n)
    try:
        for direction in m.DIRECTIONS:
            layout = (log_n + direction) & 1
            shift = m.shift_record(g, layout)
            exp = msm_pkg.host_ntt(data, root, log_n, direction, layout, shift)
            cfg.ntt_device(dom, d_in, d_out, direction, layout, shift)
            got = cfg.to_host(d_out, 32 * n)
            assert first_difference(got, exp) is None, direction
            if log_n <= 15:
                model = m.encode(m.transform(values_of(data, layout), root, log_n, direction, g), layout)
                assert first_difference(got, model) is None, direction
            if direction == m.FORWARD:                   # the round trip, in place
                cfg.ntt_device(dom, d_out, d_out, m.INVERSE, layout, shift)
                assert first_difference(cfg.to_host(d_out, 32 * n), data) is None
        assert cfg.to_host(d_in, 32 * n) == data
        sparse_check(cfg, dom, root, log_n, 1, g, log_n)
    finally:
        cfg.free(d_in)
        cfg.free(d_out)
        dom.free()


# ---- 2. tiles of 2^4 .. 2^9 elements: one, two and three passes -------------------------------------------------------------
@pytest.mark.parametrize("tile_log", shapes.MID_TILES)
def test_mid_tiles(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_NTT_TILE_LOG (read at msm_amd_init): a thread owns 1 .. 2 slots, lds_pos swizzles from 2^6 on, and the
    strided gathers of two and three passes act on small inputs"""
    monkeypatch.setenv("MSM_AMD_NTT_TILE_LOG", str(tile_log))
    c2 = msm_pkg.setup_metal_state()
    try:
        for log_n in [log_n for tl, log_n in shapes.GEOMETRY_TILES if tl == tile_log]:
            n = 1 << log_n
            n_vec = 3 if log_n <= 10 else 2
            g = 5 + log_n
            case = model_case if log_n <= MODEL_MAX_LOG else functools.partial(twin_case, msm_pkg)
            dom = c2.ntt_domain(m.H2C, log_n)
            for direction in m.DIRECTIONS:
                layout = (log_n + direction) & 1
                data, exp = case(700 + log_n, log_n, n_vec, direction, layout, g)
                got = device_ntt(c2, dom, data, direction, layout, m.shift_record(g, layout), n_vec, in_place=bool(log_n & 1))
                assert first_difference(got, exp) is None, (log_n, direction)
            direction = log_n & 1
            data, exp = case(700 + log_n, log_n, n_vec, direction, m.MONT_LE, None)
            assert first_difference(c2.ntt(dom, data, direction, m.MONT_LE, None, n_vec), exp) is None, (log_n, "no shift")
            if log_n > MODEL_MAX_LOG:
                sparse_check(c2, dom, m.H2C, log_n, n_vec, g, log_n)
            dom.free()
    finally:
        c2.close()


# ---- 3. the state after each pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_log,log_n", shapes.TAPS)
def test_pass_taps(cfg, msm_pkg, monkeypatch, tile_log, log_n):
    """msm_amd_test_ntt_passes: after p passes the pass buffer holds the network after the levels those passes cover --
    a wrong multi-pass transform names its pass"""
    plan = msm_pkg.test_ntt_plan(log_n, tile_log)
    assert len(plan) >= 2
    n = 1 << log_n
    n_vec = 2 if log_n <= MODEL_MAX_LOG else 1
    root = log_n & 1
    g = random.Random(77 + log_n).randrange(2, R)
    if tile_log != shapes.DEFAULT_TILE:
        monkeypatch.setenv("MSM_AMD_NTT_TILE_LOG", str(tile_log))
    c = cfg if tile_log == shapes.DEFAULT_TILE else msm_pkg.setup_metal_state()
    try:
        dom = c.ntt_domain(root, log_n)
        for direction in m.DIRECTIONS:
            layout = (log_n + direction) & 1
            shift = m.shift_record(g, layout)
            if log_n <= MODEL_MAX_LOG:
                a = m.random_vector(1500 + log_n, n_vec * n)
                data = m.encode(a, layout)
                states = [list(m.level_states(a[v * n:(v + 1) * n], root, log_n, direction, g)) for v in range(n_vec)]
            else:
                data = dense_records(1500 + log_n, n_vec * n)
            levels = 0
            for passes in range(1, len(plan)):
                levels += plan[passes - 1]["levels"]
                if log_n <= MODEL_MAX_LOG:
                    exp = m.encode([x for v in range(n_vec) for x in states[v][levels]], m.MONT_LE)
                else:
                    exp = msm_pkg.test_host_ntt_levels(data, root, log_n, levels, direction, layout, shift, n_vec)
                if passes == 1 and direction == m.INVERSE:
                    c.test_fill_workspaces(0xFF)
                got = c.test_ntt_passes(dom, data, passes, direction, layout, shift, n_vec)
                assert first_difference(got, exp) is None, (direction, passes)
            full = c.test_ntt_passes(dom, data, len(plan), direction, layout, shift, n_vec)
            assert first_difference(full, c.ntt(dom, data, direction, layout, shift, n_vec)) is None, direction
        dom.free()
    finally:
        if c is not cfg:
            c.close()


def test_pass_tap_argument_errors(cfg, msm_pkg):
    import ctypes
    L = msm_pkg.lib()
    log_n = 11                                       # two passes
    data = m.encode(m.random_vector(3, 1 << log_n), m.MONT_LE)
    out = ctypes.create_string_buffer(b"\xA5" * len(data), len(data))
    dom, single = cfg.ntt_domain(m.ARK, log_n), cfg.ntt_domain(m.ARK, 4)
    c2 = msm_pkg.setup_metal_state()

    def call(h=None, direction=0, layout=0, shift=None, src=data, dst=out, n_vec=1, passes=1):
        return L.msm_amd_test_ntt_passes(cfg.h, (h or dom).h, direction, layout, shift, src, dst, n_vec, passes)

    try:
        other = c2.ntt_domain(m.ARK, log_n)
        bad = msm_pkg.INPUT_ERROR
        assert call(passes=0) == bad and call(passes=3) == bad and call(passes=0xFFFFFFFF) == bad
        assert call(h=single, passes=2) == bad and call(h=other) == bad
        assert call(direction=2) == bad and call(layout=msm_pkg.SCALAR_CANON_BE32) == bad
        assert call(shift=bytes(32)) == bad and call(src=None) == bad and call(dst=None) == bad
        assert call(n_vec=1 << 21) == bad
        assert call(passes=0, n_vec=0) == bad
        assert call(n_vec=0, src=None, dst=None) == msm_pkg.OK
        assert out.raw == b"\xA5" * len(data)
        assert L.msm_amd_test_ntt_passes(None, dom.h, 0, 0, None, data, out, 1, 1) == bad
        assert call(h=single, src=data[:512], passes=1) == msm_pkg.OK     # one pass: the transform
        assert out.raw[:512] == cfg.ntt(single, data[:512]) and out.raw[512:] == b"\xA5" * (len(data) - 512)
        other.free()
    finally:
        c2.close()
        dom.free()
        single.free()


# ---- 4. the twiddle table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("root", m.ROOTS)
def test_twiddles_small(cfg, msm_pkg, root):
    for log_n in range(MODEL_MAX_LOG + 1):
        half = (1 << log_n) // 2
        w = m.omega(root, log_n)
        exp, t = [], 1
        for _ in range(half):
            exp.append(t)
            t = t * w % R
        dom = cfg.ntt_domain(root, log_n)
        try:
            assert first_difference(cfg.test_ntt_twiddles(dom, 0, half), m.encode(exp, m.MONT_LE)) is None, log_n
            if half >= 4:
                assert cfg.test_ntt_twiddles(dom, half - 3, 3) == m.encode(exp[-3:], m.MONT_LE)
        finally:
            dom.free()


@pytest.mark.parametrize("root", m.ROOTS)
def test_twiddles_large(cfg, msm_pkg, root):
    log_n = 21
    half = 1 << (log_n - 1)
    js = set(random.Random(2100 + root).sample(range(half), 4096)) | {0, 1, half - 1}
    js |= {1 << k for k in range(log_n - 1)} | {(1 << k) - 1 for k in range(log_n)}
    w = m.omega(root, log_n)
    dom = cfg.ntt_domain(root, log_n)
    try:
        table = cfg.test_ntt_twiddles(dom, 0, half)
        for j in sorted(js):
            assert table[32 * j:32 * j + 32] == m.encode([pow(w, j, R)], m.MONT_LE), j
    finally:
        dom.free()


def test_twiddle_argument_errors(cfg, msm_pkg):
    import ctypes
    L = msm_pkg.lib()
    dom = cfg.ntt_domain(m.ARK, 5)                   # 16 entries
    points, _ = msm_pkg.generate_instance_host(5, 16)
    tables = cfg.tables_build(points, 16)
    out = ctypes.create_string_buffer(b"\xA5" * 512, 512)
    bad = msm_pkg.INPUT_ERROR
    try:
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 0, 17, out) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 16, 1, out) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 17, 0, out) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 1, (1 << 64) - 1, out) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 0, 1, None) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, tables, 0, 1, out) == bad
        assert L.msm_amd_test_ntt_twiddles(None, dom.h, 0, 1, out) == bad
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 16, 0, None) == msm_pkg.OK
        assert out.raw == b"\xA5" * 512
        assert L.msm_amd_test_ntt_twiddles(cfg.h, dom.h, 15, 1, out) == msm_pkg.OK
        assert out.raw[:32] == m.encode([pow(m.omega(m.ARK, 5), 15, R)], m.MONT_LE) and out.raw[32:] == b"\xA5" * 480
    finally:
        cfg.tables_free(tables)
        dom.free()


# ---- 5. edge records and shifts on the device ---------------------------------------------------------------------------------
def raw_records(words):
    return b"".join(w.to_bytes(32, "little") for w in words)


@pytest.mark.parametrize("log_n", [3, 11])
@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_edge_records_on_the_device(cfg, msm_pkg, log_n, layout):
    n = 1 << log_n
    edge = list(dict.fromkeys(fr_ref.UNREDUCED + (0, R - 1, R, R + 1, (1 << 256) - 1)))     # seven distinct values
    rng = random.Random(log_n)
    words = [edge[i % len(edge)] if i < 2 * len(edge) or i % 3 == 0 else rng.getrandbits(256) for i in range(n)]
    data = raw_records(words)
    a = values_of(data, layout)
    assert any(w >= R for w in words) and len(a) == n
    w = m.omega(m.ARK, log_n)
    dom = cfg.ntt_domain(m.ARK, log_n)

    def run(records, direction, shift=None):
        return device_ntt(cfg, dom, records, direction, layout, shift)

    try:
        for direction in m.DIRECTIONS:
            for g in (None, 7):
                exp = m.encode(m.transform(a, m.ARK, log_n, direction, g or 1), layout)
                assert first_difference(run(data, direction, m.shift_record(g, layout)), exp) is None, (direction, g)
            assert run(bytes(32 * n), direction, m.shift_record(7, layout)) == bytes(32 * n)
            # shifts: raw records, read like an input -- the last two are >= r
            for g_raw in (m.encode([1], layout), m.encode([R - 1], layout), raw_records([R + 2]), raw_records([(1 << 256) - 1])):
                g = values_of(g_raw, layout)[0]
                exp = m.encode(m.transform(a, m.ARK, log_n, direction, g), layout)
                assert first_difference(run(data, direction, g_raw), exp) is None, (direction, g_raw.hex())
        const = 0x1234567890ABCDEF1234567890ABCDEF
        assert run(m.encode([const] * n, layout), m.FORWARD) == m.encode([n * const % R] + [0] * (n - 1), layout)
        e1 = m.encode([0, 1] + [0] * (n - 2), layout)
        assert first_difference(run(e1, m.FORWARD), m.encode([pow(w, k, R) for k in range(n)], layout)) is None
        for zero_shift in (raw_records([R]), bytes(32)):
            with pytest.raises(msm_pkg.MsmError) as e:
                run(data, m.FORWARD, zero_shift)
            assert e.value.status == msm_pkg.INPUT_ERROR, e.value
    finally:
        dom.free()


# ---- 6. batches that end inside a workgroup -----------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,n_vec", [(0, 1), (0, 1025), (3, 5), (7, 11), (9, 3), (10, 3), (13, 3)])
def test_ragged_batches(cfg, msm_pkg, log_n, n_vec):
    n = 1 << log_n
    size = 32 * n_vec * n
    tail = 32 * 64
    a = m.random_vector(1600 + log_n, n_vec * n)
    g = 1600 + log_n
    root = log_n & 1
    dom = cfg.ntt_domain(root, log_n)
    d_in, d_out = cfg.alloc(size), cfg.alloc(size + tail)
    try:
        for direction in m.DIRECTIONS:
            layout = (log_n + direction) & 1
            data, shift = m.encode(a, layout), m.shift_record(g, layout)
            singles = m.encode([x for v in range(n_vec) for x in m.transform(a[v * n:(v + 1) * n], root, log_n, direction, g)],
                               layout)
            cfg.to_device(d_in, data)
            cfg.to_device(d_out, b"\xFF" * (size + tail))
            cfg.ntt_device(dom, d_in, d_out, direction, layout, shift, n_vec)
            got = cfg.to_host(d_out, size + tail)
            assert first_difference(got[:size], singles) is None, direction
            assert got[size:] == b"\xFF" * tail, direction                     # no byte past the batch
            assert cfg.to_host(d_in, size) == data
            cfg.to_device(d_out, data + b"\xFF" * tail)
            cfg.ntt_device(dom, d_out, d_out, direction, layout, shift, n_vec)  # in place
            got = cfg.to_host(d_out, size + tail)
            assert first_difference(got[:size], singles) is None, direction
            assert got[size:] == b"\xFF" * tail, direction
    finally:
        cfg.free(d_in)
        cfg.free(d_out)
        dom.free()
