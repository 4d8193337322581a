"""The lookup calls on the GPU (msm_amd_fr_lookup_*, msm_amd_fr_prefix_sum*, msm_amd_fr_shift*) against the host twin and
the big-integer model of tests/lookup_ref.py (tests/test_lookup_host.py pins the twin to the model on the CPU).  Every
comparison is of bytes: device call = host-buffer call = twin = model.  MSM_AMD_LOOKUP_HASH_BITS shortens the hash so that
the chains of the index get long and wrap around the end of the slot array; MSM_AMD_LOOKUP_COUNT selects the counting
form.  No byte of a result depends on either."""
import random
import struct

import pytest

import fr_ref
import lookup_ref as lr

pytestmark = pytest.mark.gpu

R = lr.R


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


def unpack_idx(data):
    return list(struct.unpack("<%dI" % (len(data) // 4), data))


def check(cfg, msm_pkg, table, data, layout, n_vec=1, tag=None):
    """device call = host-buffer call = twin = model in both modes, from a handle built from host rows and one built from
    device rows; m starts as 0xFF bytes and stays so when STRICT meets a miss; the inputs are left as they were"""
    n_rows, total = len(table) // 32, len(data) // 32
    n = total // n_vec
    exp_m, exp_idx, exp_rep = lr.multiplicities(table, data, layout)
    twin = msm_pkg.host_fr_lookup_multiplicities(table, data, msm_pkg.LOOKUP_COUNT_MISSING, layout, n_vec)
    assert twin == (exp_m, exp_idx, exp_rep), tag
    dev = Device(cfg)
    d_table = dev.put(table)
    handles = [cfg.fr_lookup_build(table, layout), cfg.fr_lookup_build_device(d_table, n_rows, layout)]
    cfg.to_device(d_table, b"\xEE" * len(table))                 # the handle keeps its own copy of the rows
    try:
        infos = [h.info() for h in handles]
        for info in infos:
            assert info["n_rows"] == n_rows and info["capacity"] >= 2 * n_rows, tag
            assert info["capacity"] & (info["capacity"] - 1) == 0, tag
            assert info["device_bytes"] == msm_pkg.test_fr_lookup_plan(n_rows)["bytes"], tag
            assert 1 <= info["longest_probe"] <= info["capacity"], tag
            assert info["n_distinct"] == lr.n_distinct(table, layout), tag
        assert handles[1].build_ms >= 0
        d_in = dev.put(data)
        d_m, d_idx = dev.put(b"\xFF" * (32 * n_rows)), dev.put(b"\xFF" * (4 * max(1, total)))
        for h in handles:
            for mode in (msm_pkg.LOOKUP_COUNT_MISSING, msm_pkg.LOOKUP_STRICT):
                fails = mode == msm_pkg.LOOKUP_STRICT and exp_rep["n_missing"] != 0
                cfg.to_device(d_m, b"\xFF" * (32 * n_rows))
                cfg.to_device(d_idx, b"\xFF" * (4 * max(1, total)))
                if fails:
                    with pytest.raises(msm_pkg.MsmError) as e:
                        cfg.fr_lookup_multiplicities_device(h, d_in, n, d_m, d_idx, mode, layout, n_vec)
                    assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep, (tag, e.value)
                    assert str(exp_rep["first_missing"]) in str(e.value), e.value
                    assert dev.get(d_m, 32 * n_rows) == b"\xFF" * (32 * n_rows), tag      # untouched
                    with pytest.raises(msm_pkg.MsmError) as e:
                        cfg.fr_lookup_multiplicities(h, data, mode, layout, n_vec)
                    assert e.value.report == exp_rep and e.value.idx == exp_idx, tag
                else:
                    rep, ms = cfg.fr_lookup_multiplicities_device(h, d_in, n, d_m, d_idx, mode, layout, n_vec)
                    assert ms >= 0 and rep == exp_rep, (tag, rep, exp_rep)
                    assert lr.first_difference(dev.get(d_m, 32 * n_rows), exp_m) is None, tag
                    assert cfg.fr_lookup_multiplicities(h, data, mode, layout, n_vec) == (exp_m, exp_idx, exp_rep), tag
                    m_only = cfg.fr_lookup_multiplicities(h, data, mode, layout, n_vec, want_idx=False)
                    assert m_only == (exp_m, None, exp_rep), tag
                if total:
                    assert unpack_idx(dev.get(d_idx, 4 * total)) == exp_idx, tag
            assert dev.get(d_in, len(data)) == data and h.info() in infos, tag
    finally:
        for h in handles:
            h.free()
        dev.close()
    return infos[1]


# ---- 1. sizes, layouts, words that are equal mod r, duplicates, misses -----------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 257])
def test_sizes(cfg, msm_pkg, n_rows):
    for layout in lr.LAYOUTS:
        table = lr.random_table(n_rows + layout, n_rows, layout)
        for n, n_vec in ((1, 1), (63, 1), (64, 3), (65, 1), (257, 3), (1000, 1)):
            check(cfg, msm_pkg, table, lr.draws(n, table, layout, n * n_vec), layout, n_vec, (n_rows, layout, n, n_vec))


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_edge_words_duplicates_and_misses(cfg, msm_pkg, layout):
    edge = lr.edge_records(layout)
    table = edge + lr.encode([5, 7], layout)
    data = lr.encode(lr.decode(table, layout), layout) + edge + lr.raw([R + 5, 5])
    check(cfg, msm_pkg, table, data, layout, tag="edge")
    rng = random.Random(3)
    vals = [rng.randrange(R) for _ in range(40)]
    pairs = lr.encode([v for v in vals for _ in (0, 1)], layout)
    run = lr.encode(vals[:10] + [vals[3]] * 64 + vals[10:], layout)
    for name, table in (("pairs", pairs), ("run of 64", run)):
        check(cfg, msm_pkg, table, lr.draws(4, table, layout, 300), layout, tag=name)
        check(cfg, msm_pkg, table, lr.draws(5, table, layout, 300, (299,)), layout, tag=name + ", one miss")
        check(cfg, msm_pkg, table, lr.draws(6, table, layout, 300, (7, 64, 200)), layout, 3, tag=name + ", three misses")
    check(cfg, msm_pkg, pairs, lr.draws(7, pairs, layout, 130, tuple(range(130))), layout, tag="all missing")
    check(cfg, msm_pkg, table, b"", layout, tag="no inputs")


# ---- 2. the knob: chains that wrap; races for one slot and one counter -----------------------------------------------------------
@pytest.fixture(params=["default", "3", "0"])
def hash_bits(monkeypatch, request):
    if request.param != "default":
        monkeypatch.setenv("MSM_AMD_LOOKUP_HASH_BITS", request.param)
    return request.param


@pytest.mark.parametrize("count", ["block", "wave", "lane"])
def test_hash_bits_give_the_same_bytes(cfg, msm_pkg, hash_bits, count, monkeypatch):
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    table = lr.random_table(41, 257, lr.MONT_LE)
    data = lr.draws(42, table, lr.MONT_LE, 600, (599,))
    info = check(cfg, msm_pkg, table, data, lr.MONT_LE, tag=(hash_bits, count))
    assert info["capacity"] == 1024
    if hash_bits == "0":
        assert info["longest_probe"] == 257                   # one chain from the last slot: the last insert walked all of it
    elif hash_bits == "3":
        assert info["longest_probe"] >= 257 // 8              # eight chains at the top of the array, the first one wraps
    dup = lr.random_table(43, 257, lr.CANON_LE, distinct=9)
    check(cfg, msm_pkg, dup, lr.draws(44, dup, lr.CANON_LE, 600), lr.CANON_LE, 2, tag=(hash_bits, count, "duplicates"))


@pytest.mark.parametrize("count", ["block", "wave", "lane"])
def test_one_slot_one_counter(cfg, msm_pkg, count, monkeypatch):
    """4096 equal rows, 4096 equal inputs: every lane of every wave races for one slot and one counter"""
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    table = lr.encode([12345] * 4096, lr.MONT_LE)
    info = check(cfg, msm_pkg, table, table, lr.MONT_LE, tag="all equal")
    assert info["n_distinct"] == 1 and info["longest_probe"] == 1
    h = cfg.fr_lookup_build(table)
    try:
        m, idx, rep = cfg.fr_lookup_multiplicities(h, table)
        assert set(idx) == {0} and rep == dict(n_missing=0, first_missing=lr.NO_MISS, rows_hit=1, max_multiplicity=4096)
        assert lr.decode(m, lr.MONT_LE) == [4096] + [0] * 4095
    finally:
        h.free()
    rng = random.Random(8)
    spread = lr.random_table(9, 4096, lr.MONT_LE)
    rows = lr.decode(spread, lr.MONT_LE)
    half = [rows[0] if i % 2 else rng.choice(rows) for i in range(1 << 14)]     # half the inputs equal, half spread
    check(cfg, msm_pkg, spread, lr.encode(half, lr.MONT_LE), lr.MONT_LE, tag="half equal, 2^12 rows, 2^14 inputs")


# ---- 3. the same call twice, stale workspaces, a busy ctx, arguments, handles ------------------------------------------------------
def test_repeat_poisoned_workspaces_and_bounded_wait(msm_pkg):
    c2 = msm_pkg.setup_metal_state()
    dev = Device(c2)
    table = lr.random_table(51, 300, lr.MONT_LE, distinct=200)
    data = lr.draws(52, table, lr.MONT_LE, 700)
    exp_m, exp_idx, exp_rep = lr.multiplicities(table, data, lr.MONT_LE)
    h = c2.fr_lookup_build(table)
    try:
        d_in, d_m, d_idx = dev.put(data), dev.put(bytes(32 * 300)), dev.put(bytes(4 * 700))
        for byte in (None, 0xFF, 0x00, 0x5A):                  # the first two rounds: the same call twice
            if byte is not None:
                c2.test_fill_workspaces(byte)
            assert c2.fr_lookup_multiplicities_device(h, d_in, 700, d_m, d_idx)[0] == exp_rep, byte
            assert dev.get(d_m, 32 * 300) == exp_m and unpack_idx(dev.get(d_idx, 4 * 700)) == exp_idx, byte
            if byte is not None:
                c2.test_fill_workspaces(byte)
            assert c2.fr_lookup_multiplicities(h, data) == (exp_m, exp_idx, exp_rep), byte
        c2.to_device(d_m, b"\xEE" * (32 * 300))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)                              # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_lookup_multiplicities_device", lambda: c2.fr_lookup_multiplicities_device(h, d_in, 700, d_m)),
                           ("msm_amd_fr_lookup_multiplicities", lambda: c2.fr_lookup_multiplicities(h, data, n_rows=300)),
                           ("msm_amd_fr_prefix_sum_device", lambda: c2.fr_prefix_sum_device(d_in, 700, d_in)),
                           ("msm_amd_fr_shift_device", lambda: c2.fr_shift_device(d_in, 700, d_in, bytes(32)))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert dev.get(d_m, 32 * 300) == b"\xEE" * (32 * 300) and dev.get(d_in, len(data)) == data   # the refused calls wrote nothing
        assert c2.fr_lookup_multiplicities_device(h, d_in, 700, d_m)[0] == exp_rep and dev.get(d_m, 32 * 300) == exp_m
        left = c2.fr_lookup_build(table)                       # not freed: msm_amd_destroy takes it
        assert left.info()["n_rows"] == 300
    finally:
        h.free()
        dev.close()
        c2.close()


def test_argument_errors_and_handles(cfg, msm_pkg, dev):
    table = lr.encode([1, 2, 3, 2], lr.MONT_LE)
    data = lr.encode([2, 2, 3, 1, 1, 1], lr.MONT_LE)
    exp = lr.multiplicities(table, data, lr.MONT_LE)

    def refused(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, (a, kw)

    d = dev.put(data + b"\xDD" * (32 * 4) + b"\xDD" * 32)        # the inputs, then room for m, then for idx
    d_m, d_idx = d + 32 * 6, d + 32 * 10
    refused(cfg.fr_lookup_build, table, msm_pkg.SCALAR_CANON_BE32)
    refused(cfg.fr_lookup_build, b"")
    refused(cfg.fr_lookup_build, None, n_rows=4)
    refused(cfg.fr_lookup_build, table, n_rows=1 << 31)
    refused(cfg.fr_lookup_build_device, 0, 4)
    refused(cfg.fr_lookup_build_device, d + 8, 4)
    refused(cfg.fr_lookup_build_device, d, 0)
    refused(cfg.fr_lookup_build_device, d, 4, msm_pkg.SCALAR_CANON_BE32)
    h, h2 = cfg.fr_lookup_build(table), cfg.fr_lookup_build(table, n_rows=3)
    mat = cfg.fr_matrix_build(1, 1, [0, 0], None, None)
    other = msm_pkg.setup_metal_state()
    try:
        call = lambda *a, **kw: cfg.fr_lookup_multiplicities_device(h, *a, **kw)   # noqa: E731
        assert call(d, 6, d_m, d_idx)[0] == exp[2] and dev.get(d_m, 32 * 4) == exp[0]
        assert call(d, 3, d_m, d_idx, n_vec=2)[0] == exp[2] and call(d, 6, d_m)[0] == exp[2]
        refused(call, d, 6, d_m, d_idx, 2)                       # an unknown mode
        refused(call, d, 6, d_m, d_idx, -1)
        refused(call, d, 6, d_m, d_idx, 0, msm_pkg.SCALAR_CANON_BE32)
        refused(call, 0, 6, d_m, d_idx)
        refused(call, d, 6, 0, d_idx)
        refused(call, d + 8, 6, d_m, d_idx)                      # not 16-byte aligned
        refused(call, d, 6, d_m + 8, d_idx)
        refused(call, d, 6, d_m, d_idx + 2)
        refused(call, d, 6, d + 32 * 5, d_idx)                   # m's first record is the last input
        refused(call, d + 32 * 3, 6, d, d_idx)                   # m's last record is the first input
        refused(call, d, 6, d)
        refused(call, d, 6, d_m, d + 32 * 6 - 16)                # idx over the inputs, over m
        refused(call, d, 6, d_m, d_m + 32 * 4 - 16)
        refused(call, d, 1 << 32, d_m)
        refused(call, d, 1 << 16, d_m, n_vec=1 << 16)
        refused(cfg.fr_lookup_multiplicities, h, None, n_rows=4)
        cfg.to_device(d_m, b"\xFF" * (32 * 4))
        zero = dict(n_missing=0, first_missing=0, rows_hit=0, max_multiplicity=0)
        assert call(0, 0, d_m)[0] == zero and dev.get(d_m, 32 * 4) == bytes(32 * 4)          # no inputs: m all zero
        assert call(0, 5, d_m, n_vec=0)[0] == zero
        assert cfg.fr_lookup_multiplicities(h, b"") == (bytes(32 * 4), [], zero)
        assert cfg.fr_lookup_multiplicities(h2, data)[0] == lr.multiplicities(table[:96], data, lr.MONT_LE)[0]
        for foreign in (mat, 0):                                 # a matrix is no lookup table, and the reverse
            refused(cfg.fr_lookup_multiplicities_device, foreign, d, 6, d_m)
            refused(cfg.fr_lookup_multiplicities, foreign, data, n_rows=4)
            refused(cfg.fr_lookup_info, foreign)
        refused(cfg.fr_lookup_free, mat)
        refused(cfg.fr_matrix_info, h.h)
        refused(other.fr_lookup_multiplicities, h, data, n_rows=4)   # a handle of another ctx
        refused(other.fr_lookup_info, h)
        refused(other.fr_lookup_free, h)
        gone = other.fr_lookup_build(table)
        other.close()                                            # msm_amd_destroy frees what is left ...
        other = None
        refused(cfg.fr_lookup_info, gone)                        # ... and the handle is nobody's
        h.free()
        refused(call, d, 6, d_m)                                 # a freed handle
        refused(cfg.fr_lookup_multiplicities, h, data, n_rows=4)
        refused(h.info)
        refused(h.free)
        assert cfg.fr_lookup_multiplicities(h2, data, msm_pkg.LOOKUP_COUNT_MISSING)[2]["n_missing"] == 0
        assert dev.get(d, len(data)) == data
    finally:
        h2.free()
        mat.free()
        if other is not None:
            other.close()


# ---- 4. running sums and the shift -----------------------------------------------------------------------------------------------
@pytest.fixture
def tiles_of_four(msm_pkg, monkeypatch):
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", "2")
    c2 = msm_pkg.setup_metal_state()
    yield c2
    c2.close()


def prefix_sum_agrees(c, msm_pkg, n, n_vec, layout, seed):
    rng = random.Random(seed)
    data = lr.encode([rng.randrange(R) for _ in range(n * n_vec)], layout)
    if n > 2:
        data = lr.raw([R, (1 << 256) - 1]) + data[64:]
    dev = Device(c)
    try:
        d_in, d_out = dev.put(data), dev.put(b"\xFF" * len(data))
        for mode in (lr.INCLUSIVE, lr.EXCLUSIVE):
            exp = lr.prefix_sum(data, layout, mode, n_vec)
            assert msm_pkg.host_fr_prefix_sum(data, mode, layout, n_vec) == exp
            assert c.fr_prefix_sum_device(d_in, n, d_out, mode, layout, n_vec) >= 0
            assert lr.first_difference(dev.get(d_out, len(data)), exp) is None, (n, n_vec, mode)
            assert dev.get(d_in, len(data)) == data
            assert c.fr_prefix_sum(data, mode, layout, n_vec) == exp
            d_io = dev.put(data)                                 # in place
            c.fr_prefix_sum_device(d_io, n, d_io, mode, layout, n_vec)
            assert dev.get(d_io, len(data)) == exp
    finally:
        dev.close()


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_prefix_sum(cfg, msm_pkg, layout):
    for n, n_vec in ((1, 1), (511, 3), (512, 1), (513, 3), (2000, 2)):
        prefix_sum_agrees(cfg, msm_pkg, n, n_vec, layout, n)


def test_prefix_sum_three_and_more_levels(tiles_of_four, msm_pkg):
    for n in (17, 64, 65, 300):                                  # 4^2 < 17: three levels; 4^4 < 300: five
        assert msm_pkg.test_fr_plan(n, 3, 2)["levels"] >= 3
        prefix_sum_agrees(tiles_of_four, msm_pkg, n, 3, lr.MONT_LE, n)
    prefix_sum_agrees(tiles_of_four, msm_pkg, 300, 1, lr.CANON_LE, 1)
    data = lr.encode(list(range(1, 301)), lr.MONT_LE)            # the products of the same ctx are not disturbed
    assert tiles_of_four.fr_prefix_product(data) == fr_ref.prefix_product(data, lr.MONT_LE, lr.INCLUSIVE)


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_shift(cfg, msm_pkg, dev, layout):
    rng = random.Random(11)
    for n in (255, 256, 257):
        a = lr.raw(lr.EDGE_WORDS) + lr.encode([rng.randrange(R) for _ in range(n - 6)], layout)
        d_a, d_out = dev.put(a), dev.put(b"\xFF" * len(a))
        for kw in (0, 1, R - 1, R, (1 << 256) - 1, rng.randrange(R)):
            k = lr.raw([kw])
            exp = lr.shift(a, k, layout)
            assert msm_pkg.host_fr_shift(a, k, layout) == exp
            assert cfg.fr_shift_device(d_a, n, d_out, k, layout) >= 0
            assert lr.first_difference(dev.get(d_out, len(a)), exp) is None, (n, kw)
            assert cfg.fr_shift(a, k, layout) == exp
        d_io = dev.put(a)
        cfg.fr_shift_device(d_io, n, d_io, k, layout)            # in place
        assert dev.get(d_io, len(a)) == exp and dev.get(d_a, len(a)) == a
    with pytest.raises(msm_pkg.MsmError):
        cfg.fr_shift_device(d_a, 4, d_a + 16, k, layout)
    with pytest.raises(msm_pkg.MsmError):
        cfg.fr_shift_device(d_a, 4, d_out, None, layout)
    with pytest.raises(msm_pkg.MsmError):
        cfg.fr_map_device(6, d_a, d_a, d_a, 4, d_out, k, layout)  # no seventh op of the map
    assert cfg.fr_shift(b"", k, layout) == b""


# ---- 5. the logUp identity through the recipe of INTEGRATION.md ----------------------------------------------------------------
def test_logup_recipe(cfg, msm_pkg, dev):
    """sum_i ( sum_v 1 / (beta + f_v[i]) - m[i] / (beta + t[i]) ) = 0, every partial sum against the model, device-resident"""
    n, n_vec, L = 512, 2, lr.MONT_LE
    rng = random.Random(2024)
    t_vals = [rng.randrange(R) for _ in range(500)]
    t_vals += t_vals[:12]                                        # twelve duplicate rows: they get m = 0
    table = lr.encode(t_vals, L)
    f = lr.draws(77, table, L, n * n_vec)
    beta = rng.randrange(R)
    while any((beta + v) % R == 0 for v in t_vals):
        beta = rng.randrange(R)
    k_beta, k_one = lr.encode([beta], L), lr.encode([1], L)
    d_t, d_f = dev.put(table), dev.put(f)
    d_m, d_den, d_h = dev.put(bytes(32 * n)), dev.put(bytes(32 * n * (n_vec + 1))), dev.put(bytes(32 * n))
    h = cfg.fr_lookup_build_device(d_t, n, L)                                            # 1
    try:
        rep, _ = cfg.fr_lookup_multiplicities_device(h, d_f, n, d_m, None, msm_pkg.LOOKUP_STRICT, L, n_vec)   # 2
        assert rep["n_missing"] == 0 and rep["max_multiplicity"] < 64    # 3: the width of m for msm_amd_msm_bounded_device
        cfg.fr_shift_device(d_f, n * n_vec, d_den, k_beta, L)                            # 4: beta + f_v[i], then beta + t[i]
        cfg.fr_shift_device(d_t, n, d_den + 32 * n * n_vec, k_beta, L)
        zeros, _ = cfg.fr_batch_inverse_device(d_den, n * (n_vec + 1), d_den, L)         # 5
        assert zeros == 0
        cfg.fr_lincomb_device(d_den, n, d_h, k_one, L, n_vec)                            # 6: h_f[i] = sum_v 1 / (beta + f_v[i])
        d_ht = d_den + 32 * n * n_vec
        cfg.fr_map_device(msm_pkg.FR_MUL, d_m, d_ht, 0, n, d_ht, None, L)                # 7: h_t[i] = m[i] / (beta + t[i])
        cfg.fr_map_device(msm_pkg.FR_SUB, d_h, d_ht, 0, n, d_h, None, L)                 # 8
        cfg.fr_prefix_sum_device(d_h, n, d_h, lr.INCLUSIVE, L)                           # 9
        phi = lr.decode(dev.get(d_h, 32 * n), L)
    finally:
        h.free()
    m = lr.decode(lr.multiplicities(table, f, L)[0], L)
    fv = lr.decode(f, L)
    run, want = 0, []
    for i in range(n):
        term = sum(pow(beta + fv[v * n + i], -1, R) for v in range(n_vec)) - m[i] * pow(beta + t_vals[i], -1, R)
        run = (run + term) % R
        want.append(run)
    assert phi == want
    assert phi[-1] == 0 and any(phi)
