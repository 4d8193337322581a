"""The multilinear calls on the GPU (msm_amd_fr_mle_bind*, msm_amd_fr_mle_eval*, msm_amd_fr_eq_table*,
msm_amd_fr_sumcheck_round*) against the host twins and the big-integer model of tests/mle_ref.py (tests/test_mle_host.py
pins the twins to the model on the CPU).  Every comparison is of bytes: device call = host-buffer call = twin = model.
MSM_AMD_FR_MLE_CHUNK_LOG and MSM_AMD_FR_TILE_LOG bring every geometry -- one wave, several waves and a fold, a fold over
more than 64 partials, three and more levels of an evaluation -- down to a few thousand records."""
import ctypes
import random

import pytest

import mle_ref as m

pytestmark = pytest.mark.gpu

R = m.R
POISON = b"\xFF" * 32
BIG_LOG = 20
BIG = 1 << BIG_LOG
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


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


def n_binds(mm):
    return sorted({k for k in (1, 2, 3, mm - 1, mm) if 1 <= k <= mm})


def device_bind(dev, data, r, layout, order, n, n_vec, stride, in_place=False):
    """a bind on fresh buffers: out of place into poison, and the input must survive; returns all of the output buffer"""
    size = 32 * (m.span(n, n_vec, stride) + 3)
    d_in = dev.put(data + POISON * 3 if in_place else data)
    d_out = d_in if in_place else dev.put(POISON * (size // 32))
    assert dev.cfg.fr_mle_bind_device(d_in, n, d_out, r, order, layout, n_vec, stride) >= 0
    if not in_place:
        assert dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, size)
    dev.close()
    return out


def check_bind(c, pkg, dev, data, r_all, layout, order, n, n_vec, stride, tag, ks=None, model=True):
    """device call = host-buffer call = twin (= model); poison around and between the output tables stays"""
    mm = n.bit_length() - 1
    poison = POISON * (m.span(n, n_vec, stride) + 3)
    for k in ks or n_binds(mm):
        r = r_all[:32 * k]
        twin = m.bind_outputs(pkg.host_fr_mle_bind(data, r, n, order, layout, n_vec, stride, out=poison), n, k, n_vec, stride)
        if model:
            assert twin == m.bind(data, r, layout, order, n, n_vec, stride), (tag, k)
        places = [(False, poison)] + ([(True, data + POISON * 3)] if order == m.HIGH else [])
        for in_place, before in places:
            out = device_bind(dev, data, r, layout, order, n, n_vec, stride, in_place)
            assert m.bind_outputs(out, n, k, n_vec, stride) == twin, (tag, k, in_place)
            assert m.bind_untouched(out, before, n, n_vec, stride) is None, (tag, k, in_place)
        out = c.fr_mle_bind(data, r, n, order, layout, n_vec, stride, out=poison)
        assert m.bind_outputs(out, n, k, n_vec, stride) == twin, (tag, k)
        assert m.bind_untouched(out, poison, n, n_vec, stride) is None, (tag, k)


def device_eval(dev, data, point, layout, order, n, n_vec=1, stride=None):
    d_in = dev.put(data)
    y, ms = dev.cfg.fr_mle_eval_device(d_in, n, point, order, layout, n_vec, stride)
    assert ms >= 0 and dev.get(d_in, len(data)) == data
    dev.close()
    return y


def device_round(dev, data, layout, order, form, n, k, stride=None):
    d_in = dev.put(data)
    g, ms = dev.cfg.fr_sumcheck_round_device(d_in, n, form, order, layout, k, stride)
    assert ms >= 0 and dev.get(d_in, len(data)) == data
    dev.close()
    return g


def device_eq(dev, point, layout, order):
    mm = len(point) // 32
    d_out = dev.put(POISON * ((1 << mm) + 2))
    assert dev.cfg.fr_eq_table_device(d_out, point, order, layout) >= 0
    out = dev.get(d_out, 32 * ((1 << mm) + 2))
    dev.close()
    assert out[32 << mm:] == POISON * 2
    return out[:32 << mm]


def check_values(c, pkg, dev, mm, order, layout, model=True):
    """eval, eq table and the five round shapes at n = 2^mm: device = host-buffer call = twin (= model)"""
    n = 1 << mm
    tag = (mm, order, layout)
    point = m.challenges(mm, mm, layout)
    for n_vec, stride in ((1, n), (3, n + 5)):
        data = m.pack([m.random_values(100 * mm + v, n) for v in range(n_vec)], layout, stride)
        twin = pkg.host_fr_mle_eval(data, point, n, order, layout, n_vec, stride)
        if model:
            assert twin == m.evaluate(data, point, layout, order, n, n_vec, stride), tag
        assert device_eval(dev, data, point, layout, order, n, n_vec, stride) == twin, tag
        assert c.fr_mle_eval(data, point, n, order, layout, n_vec, stride) == twin, tag
    twin = pkg.host_fr_eq_table(point, order, layout)
    if model:
        assert twin == m.eq_table(point, layout, order), tag
    assert m.first_difference(device_eq(dev, point, layout, order), twin) is None, tag
    assert c.fr_eq_table(point, order, layout) == twin, tag
    for form, k in m.SHAPES:
        stride = n + 5 * (k & 1)
        data = m.pack([m.random_values(7 * mm + v, n) for v in range(k)], layout, stride)
        twin = pkg.host_fr_sumcheck_round(data, n, form, order, layout, k, stride)
        if model:
            assert twin == m.round_values(data, layout, order, form, n, k, stride), (tag, form, k)
        assert device_round(dev, data, layout, order, form, n, k, stride) == twin, (tag, form, k)
        assert c.fr_sumcheck_round(data, n, form, order, layout, k, stride) == twin, (tag, form, k)


# ---- 1. small geometry: every path of every plan at a few thousand records -----------------------------------------------------
@pytest.mark.parametrize("tile_log", [2, 3])
def test_small_geometry(msm_pkg, monkeypatch, tile_log):
    """MSM_AMD_FR_MLE_CHUNK_LOG and MSM_AMD_FR_TILE_LOG are read at msm_amd_init"""
    monkeypatch.setenv("MSM_AMD_FR_MLE_CHUNK_LOG", "6")
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", str(tile_log))
    P, S, E = msm_pkg.test_fr_mle_plan, msm_pkg.MLE_CALL_ROUND, msm_pkg.MLE_CALL_EVAL
    assert P(S, 1 << 7, 2, chunk_log=6)["launches"] == 1                                            # one wave
    p = P(S, 1 << 10, 2, chunk_log=6)
    assert (p["launches"], p["first_waves"]) == (2, 8)                                              # several waves and a fold
    p = P(S, 1 << 14, 2, chunk_log=6)
    assert (p["launches"], p["first_waves"]) == (2, 128)                                            # a fold over more than 64
    assert P(E, 1 << 6, 1, tile_log=tile_log)["levels"] == (3 if tile_log == 2 else 2)
    assert P(E, 1 << 10, 3, tile_log=tile_log)["levels"] == (5 if tile_log == 2 else 4)            # three levels and more
    c2 = msm_pkg.setup_metal_state()
    dev = Device(c2)
    try:
        for mm in range(1, 11):
            n = 1 << mm
            for order in m.ORDERS:
                layout = (mm + order + tile_log) & 1
                check_values(c2, msm_pkg, dev, mm, order, layout)
                r = m.challenges(3 * mm, mm, layout)
                for n_vec, stride in ((1, n), (3, n), (3, n + 5)):
                    data = m.pack([m.random_values(mm + v, n) for v in range(n_vec)], layout, stride)
                    check_bind(c2, msm_pkg, dev, data, r, layout, order, n, n_vec, stride, (mm, order, n_vec, stride))
        n = 1 << 14
        for j, (form, k) in enumerate(m.SHAPES):
            order, layout = (j + tile_log) & 1, j & 1
            data = cached(("small14", k, layout), lambda: m.pack([m.random_values(14 + v, n) for v in range(k)], layout))
            exp = cached(("small14g", form, k, order, layout), lambda: m.round_values(data, layout, order, form, n, k))
            assert msm_pkg.host_fr_sumcheck_round(data, n, form, order, layout, k) == exp
            assert device_round(dev, data, layout, order, form, n, k) == exp
    finally:
        dev.close()
        c2.close()


# ---- 2. the default knobs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [1, 6, 7, 9, 10, 16])
def test_default_knobs(cfg, msm_pkg, dev, mm):
    n = 1 << mm
    for order in m.ORDERS:
        layout = (mm + order) & 1
        check_values(cfg, msm_pkg, dev, mm, order, layout, model=mm <= 7)
        r = m.challenges(mm, mm, layout)
        data = m.pack([m.random_values(mm + v, n) for v in range(3)], layout, n + 5)
        check_bind(cfg, msm_pkg, dev, data, r, layout, order, n, 3, n + 5, (mm, order), ks=sorted({1, min(mm, 4), mm}),
                   model=mm <= 7)


@pytest.mark.parametrize("mm", [18, 19])
def test_eval_on_both_sides_of_the_level_edge(cfg, msm_pkg, dev, mm):
    n = 1 << mm
    assert msm_pkg.test_fr_mle_plan(msm_pkg.MLE_CALL_EVAL, n)["levels"] == mm - 16
    data = cached(("edge", mm), lambda: m.raw(random.Random(mm).choices(m.random_values(mm, 257), k=n)))
    for order in m.ORDERS:
        point = m.challenges(order, mm, m.MONT_LE)
        assert device_eval(dev, data, point, m.MONT_LE, order, n) == msm_pkg.host_fr_mle_eval(data, point, n, order, m.MONT_LE,
                                                                                             threads=16)


# ---- 3. 2^20 once per call: against the twin and against a closed form that needs neither -------------------------------------------
def big_affine():
    """f[i] = c + sum_j c_j bit_j(i), canonical records, and its coefficients"""
    def make():
        cs = m.random_values(20, BIG_LOG + 1)
        f = [cs[0]]
        for j in range(BIG_LOG):
            f += [(x + cs[1 + j]) % R for x in f]
        return cs, m.raw(f)
    return cached("affine", make)


def test_big_eval_and_bind_of_an_affine_table(cfg, msm_pkg, dev):
    cs, data = big_affine()
    layout = m.CANON_LE
    d_in = dev.put(data)
    for order in m.ORDERS:
        pv = m.random_values(21 + order, BIG_LOG)
        point = m.encode(pv, layout)
        y, ms = cfg.fr_mle_eval_device(d_in, BIG, point, order, layout)
        exp = (cs[0] + sum(cs[1 + m.variable(order, s, BIG_LOG)] * pv[s] for s in range(BIG_LOG))) % R
        assert ms > 0 and y == m.encode([exp], layout)
        assert y == msm_pkg.host_fr_mle_eval(data, point, BIG, order, layout, threads=16)
        # four steps (two launches): what is left is the affine table of the other sixteen variables
        d_out = dev.put(POISON * (BIG // 2 + 1))
        assert cfg.fr_mle_bind_device(d_in, BIG, d_out, point[:128], order, layout) > 0
        out = dev.get(d_out, 32 * (BIG // 2 + 1))
        assert out[32 * (BIG // 2):] == POISON
        left = out[:32 * (BIG >> 4)]
        assert m.first_difference(left, msm_pkg.host_fr_mle_bind(data, point[:128], BIG, order, layout, threads=16)[:len(left)]) is None
        bound = [m.variable(order, s, BIG_LOG) for s in range(4)]
        free = [j for j in range(BIG_LOG) if j not in bound]
        base = (cs[0] + sum(cs[1 + j] * pv[s] for s, j in enumerate(bound))) % R
        for i in [0, 1, (BIG >> 4) - 1] + random.Random(3).sample(range(BIG >> 4), 29):
            assert left[32 * i:32 * i + 32] == m.encode([base + sum(cs[1 + j] for b, j in enumerate(free) if i >> b & 1)], layout), i
    assert dev.get(d_in, len(data)) == data


@pytest.mark.parametrize("value", [1, R - 1])
def test_big_round_of_constant_tables(cfg, msm_pkg, dev, value):
    """tables that are all 1 or all r - 1: g(t) = h (+-1)^k for PRODUCT"""
    layout, h = m.MONT_LE, BIG // 2
    data = m.encode([value], layout) * (BIG * 4)
    d_in = dev.put(data)
    for order in m.ORDERS:
        for k in (1, 2, 3, 4):
            g, ms = cfg.fr_sumcheck_round_device(d_in, BIG, m.PRODUCT, order, layout, k)
            assert ms > 0 and g == m.encode([h * pow(value, k, R)] * (k + 1), layout), (order, k)
        g, _ = cfg.fr_sumcheck_round_device(d_in, BIG, m.EQ_AB_C, order, layout, 4)
        assert g == m.encode([h * value * (value * value - value)] * 4, layout)
    assert cfg.fr_sumcheck_round_device(d_in, BIG, m.EQ_AB_C, m.HIGH, layout, 4)[0] == \
        msm_pkg.host_fr_sumcheck_round(data, BIG, m.EQ_AB_C, m.HIGH, layout, 4, threads=16)


def test_big_eq_table_and_its_identities(cfg, msm_pkg, dev):
    layout = m.MONT_LE
    d_buf = dev.put(bytes(64 * BIG))                # two tables
    rng = random.Random(8)
    for order in m.ORDERS:
        pv = m.random_values(30 + order, BIG_LOG)
        point = m.encode(pv, layout)
        assert cfg.fr_eq_table_device(d_buf, point, order, layout) > 0
        eq = dev.get(d_buf, 32 * BIG)
        for i in [0, 1, 1 << 19, BIG - 1] + rng.sample(range(BIG), 64):
            assert eq[32 * i:32 * i + 32] == m.encode([m.eq_entry(pv, order, i)], layout), (order, i)
        assert m.first_difference(eq, msm_pkg.host_fr_eq_table(point, order, layout, threads=16)) is None
        # sum eq = 1 through a PRODUCT round of one table
        g = m.decode(cfg.fr_sumcheck_round_device(d_buf, BIG, m.PRODUCT, order, layout, 1)[0], layout)
        assert (g[0] + g[1]) % R == 1
        # sum eq f = eval(f) through a PRODUCT round of two: f is the eq table of another point, in table 1
        qv = m.random_values(40 + order, BIG_LOG)
        q = m.encode(qv, layout)
        cfg.fr_eq_table_device(d_buf + 32 * BIG, q, order, layout)
        g = m.decode(cfg.fr_sumcheck_round_device(d_buf, BIG, m.PRODUCT, order, layout, 2)[0], layout)
        y, _ = cfg.fr_mle_eval_device(d_buf + 32 * BIG, BIG, point, order, layout)
        assert m.encode([g[0] + g[1]], layout) == y
        closed = 1                                  # eq(q, .) at p = prod (p q + (1 - p)(1 - q))
        for a, b in zip(pv, qv):
            closed = closed * (a * b + (1 - a) * (1 - b)) % R
        assert y == m.encode([closed], layout)


# ---- 4. the protocol, on the device from the first round to the last ------------------------------------------------------------------
@pytest.mark.parametrize("form,k", [(m.EQ_AB_C, 4), (m.PRODUCT, 3)])
def test_protocol_on_the_device(cfg, msm_pkg, dev, form, k):
    mm, layout = 12, m.MONT_LE
    n0 = 1 << mm
    tabs = cached(("proto", k), lambda: [m.random_values(12 + v, n0) for v in range(k)])
    data = m.pack(tabs, layout)
    claim0 = cached(("proto-total", form, k), lambda: m.total(tabs, form))
    rs = m.random_values(99, mm)
    point = m.encode(rs, layout)
    d_orig = dev.put(data)
    # HIGH: all tables in one buffer at stride n0, bound in place
    d_t, n, claim = dev.put(data), n0, claim0
    for s in range(mm):
        g, _ = cfg.fr_sumcheck_round_device(d_t, n, form, m.HIGH, layout, k, n0)
        claim = m.verifier_step(claim, m.decode(g, layout), rs[s])
        cfg.fr_mle_bind_device(d_t, n, d_t, point[32 * s:32 * s + 32], m.HIGH, layout, k, n0)
        n //= 2
    finals = [m.decode(dev.get(d_t + 32 * v * n0, 32), layout)[0] for v in range(k)]
    assert claim == m.combine(form, finals)
    assert m.encode(finals, layout) == cfg.fr_mle_eval_device(d_orig, n0, point, m.HIGH, layout, k)[0]
    # LOW: between two buffers
    d_a, d_b, n, claim = dev.put(data), dev.put(bytes(len(data))), n0, claim0
    for s in range(mm):
        g, _ = cfg.fr_sumcheck_round_device(d_a, n, form, m.LOW, layout, k, n0)
        claim = m.verifier_step(claim, m.decode(g, layout), rs[s])
        cfg.fr_mle_bind_device(d_a, n, d_b, point[32 * s:32 * s + 32], m.LOW, layout, k, n0)
        d_a, d_b, n = d_b, d_a, n // 2
    finals = [m.decode(dev.get(d_a + 32 * v * n0, 32), layout)[0] for v in range(k)]
    assert claim == m.combine(form, finals)
    assert m.encode(finals, layout) == cfg.fr_mle_eval_device(d_orig, n0, point, m.LOW, layout, k)[0]
    assert dev.get(d_orig, len(data)) == data


# ---- 5. the recipe of INTEGRATION.md: a sumcheck over resident tables ---------------------------------------------------------------------
def test_r1cs_zero_check_recipe(cfg, msm_pkg, dev):
    """a satisfied R1CS of 2^10 rows: A z, B z, C z by one sparse product into tables 1 - 3, eq(tau, .) into table 0, claim 0"""
    mm, layout = 10, m.MONT_LE
    n0 = 1 << mm
    rng = random.Random(10)
    z = [rng.randrange(1, R) for _ in range(n0)]
    rows_a = [[(rng.randrange(n0), rng.randrange(R)) for _ in range(1 + i % 3)] for i in range(n0)]
    rows_b = [[(rng.randrange(n0), rng.choice((1, R - 1, rng.randrange(R)))) for _ in range(1 + i % 2)] for i in range(n0)]
    dot = lambda row: sum(v * z[c] for c, v in row) % R                                                    # noqa: E731
    az, bz = [dot(r) for r in rows_a], [dot(r) for r in rows_b]
    rows_c = [[(i, az[i] * bz[i] * pow(z[i], -1, R) % R)] for i in range(n0)]                               # C z = A z o B z
    rows = rows_a + rows_b + rows_c
    row_ptr, col_idx, vals = [0], [], []
    for row in rows:
        col_idx += [c for c, _ in row]
        vals += [v for _, v in row]
        row_ptr.append(len(col_idx))
    mat = cfg.fr_matrix_build(3 * n0, n0, row_ptr, col_idx, m.encode(vals, layout), layout)
    tau = m.random_values(11, mm)
    rs = m.random_values(12, mm)
    d_z = dev.put(m.encode(z, layout))
    try:
        for spoil in (False, True):
            d_t = dev.put(bytes(32 * 4 * n0))
            cfg.fr_eq_table_device(d_t, m.encode(tau, layout), m.HIGH, layout)
            cfg.fr_matvec_device(mat, d_z, d_t + 32 * n0, layout)
            assert dev.get(d_t + 32 * n0, 64 * n0) == m.encode(az + bz, layout)
            if spoil:
                cfg.to_device(d_t + 32 * (3 * n0 + 77), m.encode([az[77] * bz[77] + 1], layout))
            n, claim = n0, 0
            for s in range(mm):
                g, _ = cfg.fr_sumcheck_round_device(d_t, n, m.EQ_AB_C, m.HIGH, layout, 4, n0)
                g = m.decode(g, layout)
                if spoil:
                    assert (g[0] + g[1]) % R != 0
                    break
                claim = m.verifier_step(claim, g, rs[s])
                cfg.fr_mle_bind_device(d_t, n, d_t, m.encode([rs[s]], layout), m.HIGH, layout, 4, n0)
                n //= 2
            if not spoil:
                e, a, b, c = [m.decode(dev.get(d_t + 32 * v * n0, 32), layout)[0] for v in range(4)]
                assert claim == e * (a * b - c) % R
                assert e == m.evaluate_ints(m.eq_ints(tau, m.HIGH), m.HIGH, rs)
    finally:
        cfg.fr_matrix_free(mat)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------------
def test_stale_workspaces_change_nothing(cfg, msm_pkg, dev):
    mm, layout = 13, m.CANON_LE
    n = 1 << mm
    data = m.pack([m.random_values(9 + v, n) for v in range(4)], layout)
    point = m.challenges(9, mm, layout)

    def run():
        return (device_bind(dev, data, point[:160], layout, m.LOW, n, 4, n), device_bind(dev, data, point[:160], layout, m.HIGH, n, 4, n),
                device_eval(dev, data, point, layout, m.LOW, n, 4), device_round(dev, data, layout, m.HIGH, m.EQ_AB_C, n, 4),
                device_round(dev, data, layout, m.LOW, m.PRODUCT, n, 3), cfg.fr_mle_eval(data, point, n, m.HIGH, layout, 4),
                cfg.fr_sumcheck_round(data, n, m.PRODUCT, m.LOW, layout, 2), cfg.fr_mle_bind(data, point[:160], n, m.LOW, layout, 4))

    assert msm_pkg.test_fr_mle_plan(msm_pkg.MLE_CALL_ROUND, n, 4)["launches"] == 2          # partial records in the workspace
    assert msm_pkg.test_fr_mle_plan(msm_pkg.MLE_CALL_BIND, n, 4, n_bind=5)["records"] > 0   # and the turns of a LOW bind
    first = run()
    cfg.test_fill_workspaces(0xFF)
    assert run() == first
    cfg.test_fill_workspaces(0x00)
    assert run() == first
    assert first[2] == msm_pkg.host_fr_mle_eval(data, point, n, m.LOW, layout, 4)
    assert first[3] == msm_pkg.host_fr_sumcheck_round(data, n, m.EQ_AB_C, m.HIGH, layout, 4)
    assert m.bind_outputs(first[0], n, 5, 4, n) == m.bind_outputs(msm_pkg.host_fr_mle_bind(data, point[:160], n, m.LOW, layout, 4), n, 5, 4, n)


def test_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    mm, layout = 7, m.MONT_LE
    n = 1 << mm
    data = m.pack([m.random_values(4 + v, n) for v in range(2)], layout)
    point = m.challenges(4, mm, layout)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        d, d_o = c2.alloc(len(data)), c2.alloc(len(data))
        c2.to_device(d, data)
        c2.to_device(d_o, bytes(len(data)))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_mle_bind_device", lambda: c2.fr_mle_bind_device(d, n, d_o, point[:32], m.LOW, layout, 2)),
                           ("msm_amd_fr_mle_bind", lambda: c2.fr_mle_bind(data, point[:32], n, m.LOW, layout, 2)),
                           ("msm_amd_fr_mle_eval_device", lambda: c2.fr_mle_eval_device(d, n, point, m.LOW, layout, 2)),
                           ("msm_amd_fr_mle_eval", lambda: c2.fr_mle_eval(data, point, n, m.LOW, layout, 2)),
                           ("msm_amd_fr_eq_table_device", lambda: c2.fr_eq_table_device(d_o, point, m.LOW, layout)),
                           ("msm_amd_fr_eq_table", lambda: c2.fr_eq_table(point, m.LOW, layout)),
                           ("msm_amd_fr_sumcheck_round_device", lambda: c2.fr_sumcheck_round_device(d, n, m.PRODUCT, m.LOW, layout, 2)),
                           ("msm_amd_fr_sumcheck_round", lambda: c2.fr_sumcheck_round(data, n, m.PRODUCT, m.LOW, layout, 2))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data and c2.to_host(d_o, len(data)) == bytes(len(data))     # the refused calls wrote nothing
        assert c2.fr_mle_eval_device(d, n, point, m.LOW, layout, 2)[0] == m.evaluate(data, point, layout, m.LOW, n, 2)
        assert c2.fr_sumcheck_round(data, n, m.PRODUCT, m.LOW, layout, 2) == m.round_values(data, layout, m.LOW, m.PRODUCT, n, 2)
        c2.free(d)
        c2.free(d_o)
    finally:
        c2.close()


def test_argument_errors_and_empty_calls(cfg, msm_pkg, dev):
    L, vp = msm_pkg.lib(), ctypes.c_void_p
    n, be32 = 16, msm_pkg.SCALAR_CANON_BE32
    data = m.pack([m.random_values(v, n) for v in range(4)], m.MONT_LE)
    r = m.challenges(1, 4, m.MONT_LE)
    d_in, d_out = dev.put(data + data), dev.put(b"\xA5" * len(data))
    g = ctypes.create_string_buffer(160)
    h = cfg.h
    bind = lambda *a: ("msm_amd_fr_mle_bind_device", L.msm_amd_fr_mle_bind_device(h, *a, None))                  # noqa: E731
    ev = lambda *a: ("msm_amd_fr_mle_eval_device", L.msm_amd_fr_mle_eval_device(h, *a, None))                    # noqa: E731
    eq = lambda *a: ("msm_amd_fr_eq_table_device", L.msm_amd_fr_eq_table_device(h, *a, None))                    # noqa: E731
    rnd = lambda *a: ("msm_amd_fr_sumcheck_round_device", L.msm_amd_fr_sumcheck_round_device(h, *a, None))       # noqa: E731
    hbind = lambda *a: ("msm_amd_fr_mle_bind", L.msm_amd_fr_mle_bind(h, *a))                                     # noqa: E731
    hev = lambda *a: ("msm_amd_fr_mle_eval", L.msm_amd_fr_mle_eval(h, *a))                                       # noqa: E731
    heq = lambda *a: ("msm_amd_fr_eq_table", L.msm_amd_fr_eq_table(h, *a))                                       # noqa: E731
    hrnd = lambda *a: ("msm_amd_fr_sumcheck_round", L.msm_amd_fr_sumcheck_round(h, *a))                          # noqa: E731
    i_, o_ = vp(d_in), vp(d_out)
    hout = ctypes.create_string_buffer(len(data))
    cases = [
        lambda: bind(be32, 0, r, 1, i_, n, 1, n, o_), lambda: bind(7, 0, r, 1, i_, n, 1, n, o_),                 # layout
        lambda: ev(be32, 0, r, i_, n, 1, n, g), lambda: eq(be32, 0, r, 4, o_), lambda: rnd(be32, 0, 0, i_, n, 1, n, g),
        lambda: hbind(be32, 0, r, 1, data, n, 1, n, hout), lambda: hev(be32, 0, r, data, n, 1, n, g),
        lambda: heq(be32, 0, r, 4, hout), lambda: hrnd(be32, 0, 0, data, n, 1, n, g),
        lambda: bind(0, 2, r, 1, i_, n, 1, n, o_), lambda: ev(0, -1, r, i_, n, 1, n, g),                         # order
        lambda: eq(0, 2, r, 4, o_), lambda: rnd(0, 5, 0, i_, n, 1, n, g),
        lambda: rnd(0, 0, 2, i_, n, 1, n, g), lambda: hrnd(0, 0, -1, data, n, 1, n, g),                          # form
        lambda: rnd(0, 0, 0, i_, n, 5, n, g), lambda: rnd(0, 0, 1, i_, n, 3, n, g), lambda: rnd(0, 0, 1, i_, n, 1, n, g),
        lambda: bind(0, 0, r, 1, i_, 12, 1, 12, o_), lambda: bind(0, 0, r, 1, i_, 1, 1, 1, o_),                  # n
        lambda: bind(0, 0, r, 1, i_, 0, 1, 0, o_), lambda: ev(0, 0, r, i_, 24, 1, 24, g), lambda: rnd(0, 0, 0, i_, 1, 1, 1, g),
        lambda: ev(0, 0, r, i_, 1 << 32, 1, 1 << 32, g),
        lambda: bind(0, 0, r, 0, i_, n, 1, n, o_), lambda: bind(0, 0, r, 5, i_, n, 1, n, o_),                    # n_bind
        lambda: bind(0, 0, r, 1, i_, n, 2, n - 1, o_), lambda: ev(0, 0, r, i_, n, 2, 8, g),                      # stride < n
        lambda: rnd(0, 0, 0, i_, n, 2, n - 1, g),
        lambda: bind(0, 0, r, 1, i_, n, 1 << 16, 1 << 16, o_), lambda: ev(0, 0, r, i_, n, 1 << 28, n, g),        # n_vec stride >= 2^32
        lambda: rnd(0, 0, 0, i_, n, 2, 1 << 31, g),
        lambda: bind(0, 0, None, 1, i_, n, 1, n, o_), lambda: bind(0, 0, r, 1, None, n, 1, n, o_),               # null pointers
        lambda: bind(0, 0, r, 1, i_, n, 1, n, None), lambda: ev(0, 0, None, i_, n, 1, n, g), lambda: ev(0, 0, r, None, n, 1, n, g),
        lambda: ev(0, 0, r, i_, n, 1, n, None), lambda: eq(0, 0, None, 4, o_), lambda: eq(0, 0, r, 4, None),
        lambda: rnd(0, 0, 0, None, n, 1, n, g), lambda: rnd(0, 0, 0, i_, n, 1, n, None),
        lambda: hbind(0, 0, r, 1, None, n, 1, n, hout), lambda: hev(0, 0, r, data, n, 1, n, None),
        lambda: eq(0, 0, r, 0, o_), lambda: eq(0, 0, r, 32, o_), lambda: heq(0, 0, r, 0, hout),                  # m
        lambda: bind(0, 0, r, 1, vp(d_in + 8), n, 1, n, o_), lambda: bind(0, 0, r, 1, i_, n, 1, n, vp(d_out + 4)),   # alignment
        lambda: ev(0, 0, r, vp(d_in + 8), n, 1, n, g), lambda: eq(0, 0, r, 4, vp(d_out + 8)),
        lambda: rnd(0, 0, 0, vp(d_in + 4), n, 1, n, g),
        lambda: bind(0, 0, r, 1, i_, n, 1, n, i_),                                                               # LOW in place
        lambda: bind(0, 0, r, 1, i_, n, 1, n, vp(d_in + 32)), lambda: bind(0, 1, r, 1, i_, n, 1, n, vp(d_in + 32)),  # partial overlap
        lambda: bind(0, 1, r, 1, vp(d_in + 32), n, 1, n, i_), lambda: bind(0, 1, r, 1, i_, n, 4, n, vp(d_in + 32 * n)),
        lambda: bind(0, 0, r, 1, vp(d_in + 32 * (n // 2 - 1)), n, 1, n, i_),
    ]
    for j, case in enumerate(cases):
        name, st = case()
        assert st == msm_pkg.INPUT_ERROR, (j, name)
        assert name.encode() + b":" in L.msm_amd_last_error(h), (j, name, L.msm_amd_last_error(h))
    assert dev.get(d_out, len(data)) == b"\xA5" * len(data) and dev.get(d_in, 2 * len(data)) == data + data
    # nothing to do: OK, nothing touched
    assert bind(0, 0, None, 0, None, 12, 0, 0, None)[1] == msm_pkg.OK and ev(0, 1, None, None, 0, 0, 0, None)[1] == msm_pkg.OK
    assert rnd(0, 0, 1, None, 3, 0, 0, None)[1] == msm_pkg.OK and hbind(0, 1, None, 0, None, 0, 0, 0, None)[1] == msm_pkg.OK
    assert hev(0, 0, None, None, 0, 0, 0, None)[1] == msm_pkg.OK and hrnd(0, 0, 0, None, 0, 0, 0, None)[1] == msm_pkg.OK
    assert dev.get(d_out, len(data)) == b"\xA5" * len(data)
    # right behind the input is disjoint from it
    assert bind(0, 0, r, 1, i_, n, 4, n, vp(d_in + 32 * 4 * n))[1] == msm_pkg.OK
    assert m.bind_outputs(dev.get(d_in + 32 * 4 * n, len(data)), n, 1, 4, n) == m.bind(data, r[:32], m.MONT_LE, m.LOW, n, 4)
