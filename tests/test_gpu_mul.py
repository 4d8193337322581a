"""GPU tests of the batch scalar multiplication: the device entry, the host-buffer entry and the host twin byte for byte,
all against the big-integer models at the planted records and at 32 random positions, over lane tails, wave and
workgroup edges; whole arrays (scalar and base progressions, every table entry, the digit edges) and the G1 inputs that
take the exceptional branches, against the model at EVERY position; prepared output against the bases conversion and in an MSM; the normalisation cases; the G2 base of
order 10069; the sum identity; the chain with check / compress / decompress; isolation; chunking; the bounded wait; no
scratch.  Expected values come from mul_ref (the models), never from the library."""
import random

import pytest

import check_ref as c
import g2_ref as g
import mul_ref as m
import test_mul_host as hst

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
GROUPS = [1, 2]
MODES = [m.EACH, m.ONE]
o = c.o
_CASE = {}
_PERM = random.Random(4099).sample(range(4099), 4099)


def on_device(cfg, data):
    d = cfg.alloc(len(data))
    cfg.to_device(d, data)
    return d


def case(msm_pkg, group):
    """4099 scalars (the planted ones first) and a pool of 8 bases, base i % 8 for record i; computed once per group"""
    if group not in _CASE:
        plan = msm_pkg.mul_plan(group)
        ks, names = m.planted_scalars(plan["c"], plan["W"])
        rng = random.Random(500 + group)
        ks = ks + [rng.randrange(m.R) for _ in range(max(SIZES) - len(ks))]
        pool = [m.GEN[group]] + m.random_points(group, 6, 17) + [None]
        _CASE[group] = (ks, len(names), pool)
    return _CASE[group]


def device_mul(cfg, msm_pkg, group, mode, sc, pts, n, sl, li, lo):
    """the device entry on freshly uploaded buffers: n output records"""
    size = msm_pkg.decompressed_bytes(lo, group == 2)
    d_sc, d_pts, d_out = on_device(cfg, sc), on_device(cfg, pts), cfg.alloc(n * size)
    try:
        cfg.mul_points_device(d_sc, d_pts, n, d_out, mode, sl, li, lo, g2=group == 2)
        return cfg.to_host(d_out, n * size)
    finally:
        for p in (d_sc, d_pts, d_out):
            cfg.free(p)


def everywhere(cfg, msm_pkg, group, mode, ks, bases, sl=0, li=0, lo=0, z=1):
    """device entry == host-buffer entry == host twin; returns the bytes.  bases: one per scalar (BASE_ONE: equal)"""
    n = len(ks)
    sc = m.scalars_bytes(ks, sl)
    pts = b"".join(m.base_record(group, li, p, z) for p in (bases if mode == m.EACH else bases[:1]))
    h = msm_pkg.host_mul_points(sc, pts, n, mode, sl, li, lo, g2=group == 2)
    b = cfg.mul_points(sc, pts, n, mode, sl, li, lo, g2=group == 2)
    d = device_mul(cfg, msm_pkg, group, mode, sc, pts, n, sl, li, lo)
    assert d == h, "device entry differs from the host twin"
    assert b == h, "host-buffer entry differs from the host twin"
    return d


def assert_model(got, group, lo, ks, bases, positions):
    size = m.OUT_BYTES[(group, lo)]
    for i in positions:
        assert got[i * size:(i + 1) * size] == m.out_record(group, lo, m.expected(group, ks[i] % m.R, bases[i])), i


# ---- 1. device == host-buffer entry == host twin, and the model --------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(cfg, msm_pkg, group, mode, n):
    ks, n_planted, pool = case(msm_pkg, group)
    ks = ks[:n]
    k = SIZES.index(n)
    sl = m.SCALAR_LAYOUTS[k % 3]
    li = m.IN_LAYOUTS[group][k % len(m.IN_LAYOUTS[group])]
    lo = m.OUT_LAYOUTS[group][(k // 2) % 2]
    bases = [pool[i % 8] for i in range(n)] if mode == m.EACH else [pool[0]] * n
    got = everywhere(cfg, msm_pkg, group, mode, ks, bases, sl, li, lo, z=1 + k)
    positions = sorted(set(range(min(n, n_planted))) | set([i for i in _PERM if i < n][:32]))
    if mode == m.EACH:                                      # the planted scalars meet the generator at i % 8 == 0 only:
        positions = [i for i in positions if i % 8 in (0, 7) or i >= n_planted]      # keep those, the identity base, the rest
    assert_model(got, group, lo, ks, bases, positions)


# ---- 2. prepared output, prepared input ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_prepared_output_equals_the_bases_conversion_and_runs_an_msm(cfg, msm_pkg, group, mode):
    n, g2 = 257, group == 2
    rng = random.Random(60 + group)
    dl = [rng.randrange(1, 1 << 40) for _ in range(n)]     # s_i, small: the model's sum below stays cheap
    dl[3], dl[200] = 0, 0                                   # identity outputs among the bases of the MSM
    kk = [rng.randrange(m.R) for _ in range(n)]
    gen = m.GEN[group]
    prepared = msm_pkg.G2_POINT_PREPARED if g2 else msm_pkg.POINT_PREPARED
    psize = msm_pkg.decompressed_bytes(prepared, g2)
    d_s = on_device(cfg, m.scalars_bytes(dl, 0))
    d_base = on_device(cfg, m.base_record(group, 0, gen) * (n if mode == m.EACH else 1))
    d_prep, d_kk = cfg.alloc(n * psize), on_device(cfg, m.scalars_bytes(kk, 0))
    try:
        cfg.mul_points_device(d_s, d_base, n, d_prep, mode, 0, 0, prepared, g2=g2)
        got = cfg.to_host(d_prep, n * psize)
        for lo in m.OUT_LAYOUTS[group]:                     # both affine forms convert to the same records
            asize = msm_pkg.decompressed_bytes(lo, g2)
            d_aff = cfg.alloc(n * asize)
            try:
                cfg.mul_points_device(d_s, d_base, n, d_aff, mode, 0, 0, lo, g2=g2)
                d_ref = (cfg.g2_bases_prepare_device if g2 else cfg.bases_prepare_device)(d_aff, n, lo)
                try:
                    assert cfg.to_host(d_ref, n * psize) == got
                finally:
                    cfg.free(d_ref)
            finally:
                cfg.free(d_aff)
        # prepared INPUT: the generated array as the bases of a second multiplication
        d_again = cfg.alloc(n * psize)
        try:
            cfg.mul_points_device(d_kk, d_prep, n, d_again, m.EACH, 0, prepared, prepared, g2=g2)
            again = cfg.to_host(d_again, n * psize)
            cfg.mul_points_device(d_kk, d_prep, n, d_again, m.ONE, 0, prepared, 0, g2=g2)      # ONE prepared record
            one = cfg.to_host(d_again, 2 * msm_pkg.decompressed_bytes(0, g2))
        finally:
            cfg.free(d_again)
        if g2:
            out = cfg.msm_g2_device(d_kk, d_prep, n, point_layout=prepared)
        else:
            out = cfg.msm_batch_device([d_kk], [d_prep], [n], point_layout=prepared)[0]
    finally:
        for p in (d_s, d_base, d_prep, d_kk):
            cfg.free(p)
    total = sum(k * s for k, s in zip(kk, dl)) % m.R
    if g2:
        assert g.decode_jacobian(out) == m.expected(2, total, gen)
    else:
        assert o.decode_jacobian_mont_le(out) == m.expected(1, total, gen)
    first = m.expected(group, dl[0], gen)
    assert_model(one, group, 0, kk, [first, first], [0, 1])
    assert len(again) == n * psize and again != got


# ---- 3. the normalisation cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_batched_normalisation(cfg, msm_pkg, group, mode):
    K = msm_pkg.mul_plan(group)["K"]
    pts = m.random_points(group, 2 * K + 1, 21)
    for n in (1, K - 1, K, K + 1, 2 * K + 1):
        for whole in (False, True):
            ks = m.normalisation_case(K, n, 100 * n + whole, whole)
            bases = pts[:n] if mode == m.EACH else [pts[0]] * n
            lo = m.OUT_LAYOUTS[group][n % 2]
            got = everywhere(cfg, msm_pkg, group, mode, ks, bases, lo=lo)
            assert_model(got, group, lo, ks, bases, range(n))
    for n in (1, K, K + 1):                                 # nothing but identities
        bases = pts[:n] if mode == m.EACH else [pts[0]] * n
        assert everywhere(cfg, msm_pkg, group, mode, [0] * n, bases) == m.out_record(group, 0, None) * n


# ---- 4. the G2 base of order 10069 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_g2_base_of_order_10069(cfg, msm_pkg, mode):
    small, q = m.small_order_point(), m.ORDER_SMALL
    rng = random.Random(9)
    ks = [q, q - 1, q + 1, 2 * q, 2 * q - 1, 3 * q + 1, q * q, q << 100, (q << 100) + 1, 1, 2, 3, q // 2, q // 2 + 1]
    ks += [q * rng.randrange(1, m.R // q) for _ in range(6)] + [rng.randrange(m.R) for _ in range(12)]
    ks += [rng.randrange(1 << 20) for _ in range(65 - len(ks))]                    # more than one wave
    n = len(ks)
    bases = [small if i % 2 == 0 else g.neg(small) for i in range(n)] if mode == m.EACH else [small] * n
    got = everywhere(cfg, msm_pkg, 2, mode, ks, bases)
    assert_model(got, 2, 0, ks, bases, range(n))
    for i, k in enumerate(ks):
        assert (got[128 * i:128 * i + 128] == bytes(128)) == (k % q == 0), i


# ---- 5. the sum identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_sum_of_the_outputs(cfg, msm_pkg, group):
    n = 4099
    ks, _, pool = case(msm_pkg, group)
    gen = pool[0]
    sc = m.scalars_bytes(ks, 0)
    got = device_mul(cfg, msm_pkg, group, m.ONE, sc, m.base_record(group, 0, gen), n, 0, 0, 0)
    total = m.expected(group, sum(ks) % m.R, gen)
    if group == 1:
        one = o.fq_to_mont(1).to_bytes(32, "little")
        recs = [got[64 * i:64 * i + 64] for i in range(n)]
        jac = [r + (one if r != bytes(64) else bytes(32)) for r in recs]
        assert o.decode_jacobian_mont_le(msm_pkg.sum_points(jac)) == total
    else:
        acc = None
        for i in range(n):
            acc = g.add(acc, g.decode_h2c(got[128 * i:128 * i + 128]))
        assert acc == total


# ---- 6. the chain with the shipped calls ---------------------------------------------------------------------------------------------
def test_generated_g2_array_checks_compresses_and_decompresses(cfg, msm_pkg):
    n = 257
    ks, _, pool = case(msm_pkg, 2)
    d_s, d_base = on_device(cfg, m.scalars_bytes(ks[:n], 0)), on_device(cfg, m.base_record(2, 0, pool[1]))
    d_out, d_comp, d_back = cfg.alloc(128 * n), cfg.alloc(64 * n), cfg.alloc(128 * n)
    try:
        cfg.mul_points_device(d_s, d_base, n, d_out, m.ONE, 0, 0, 0, g2=True)
        rep = cfg.g2_check_points_device(d_out, n, checks=msm_pkg.CHECK_CURVE | msm_pkg.CHECK_SUBGROUP)
        assert rep["n_invalid"] == 0 and rep["n_checked"] == n and rep["n_identity"] == 1      # s = 0 at index 0
        for fmt in (msm_pkg.COMPRESSED_ARK, msm_pkg.COMPRESSED_PARITY):
            assert cfg.compress_points_device(d_out, n, d_comp, fmt, 0, g2=True) == 0
            back = cfg.decompress_points_device(d_comp, n, d_back, fmt, 0, g2=True)
            assert back["n_invalid"] == 0
            assert cfg.to_host(d_back, 128 * n) == cfg.to_host(d_out, 128 * n)
    finally:
        for p in (d_s, d_base, d_out, d_comp, d_back):
            cfg.free(p)


# ---- 7. isolation, stale workspaces, chunks -------------------------------------------------------------------------------------------
def test_g2_call_between_a_g1_submit_and_its_wait(cfg, msm_pkg):
    n = 1 << 12
    points, scalars = msm_pkg.generate_instance_host(o.SEED_BASE + 5, n)
    before = cfg.msm(scalars, points, n)
    ks, _, pool = case(msm_pkg, 2)
    m2 = 257
    sc2, base2 = m.scalars_bytes(ks[:m2], 0), m.base_record(2, 0, pool[2])
    want2 = msm_pkg.host_mul_points(sc2, base2, m2, m.ONE, g2=True)
    dp, ds = on_device(cfg, points), on_device(cfg, scalars)
    try:
        handle = cfg.submit_batch_device([ds], [dp], [n])
        got2 = cfg.mul_points(sc2, base2, m2, m.ONE, g2=True)
        res = cfg.wait_batch(handle)
    finally:
        cfg.free(dp)
        cfg.free(ds)
    assert got2 == want2 and res[0] == before
    assert cfg.msm(scalars, points, n) == before


@pytest.mark.parametrize("group", GROUPS)
def test_stale_workspaces_change_nothing(cfg, msm_pkg, group):
    n = 257
    ks, _, pool = case(msm_pkg, group)
    sc = m.scalars_bytes(ks[:n], 0)
    for mode in MODES:
        pts = b"".join(m.base_record(group, 0, pool[i % 8]) for i in range(n if mode == m.EACH else 1))
        first = cfg.mul_points(sc, pts, n, mode, g2=group == 2)
        cfg.test_fill_workspaces(0xFF)
        assert cfg.mul_points(sc, pts, n, mode, g2=group == 2) == first
        assert first == msm_pkg.host_mul_points(sc, pts, n, mode, g2=group == 2)


def test_chunked_call_writes_the_same_bytes(msm_pkg, monkeypatch):
    """MSM_AMD_MUL_CHUNK (read at msm_amd_init) lowers the chunk to one normalisation group: K + 1 records are the
    smallest call of two chunks; 4 K + 3 make five"""
    K = msm_pkg.mul_plan(1)["K"]
    monkeypatch.setenv("MSM_AMD_MUL_CHUNK", str(K))
    c2 = msm_pkg.setup_metal_state()
    try:
        for group in GROUPS:
            ks, _, pool = case(msm_pkg, group)
            for n in (K + 1, 4 * K + 3):
                for mode in MODES:
                    bases = [pool[i % 8] for i in range(n)] if mode == m.EACH else [pool[1]] * n
                    everywhere(c2, msm_pkg, group, mode, ks[:n], bases, lo=m.OUT_LAYOUTS[group][1])
    finally:
        c2.close()


# ---- 8. arguments, the bounded wait ------------------------------------------------------------------------------------------------------
def test_argument_errors(cfg, msm_pkg):
    def input_error(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, e.value

    n = 8
    sc, p1, p2 = bytes(32 * n), m.base_record(1, 0, o.GEN) * n, m.base_record(2, 0, g.GEN2) * n
    d_sc, d1, d2, d_out = on_device(cfg, sc), on_device(cfg, p1), on_device(cfg, p2), cfg.alloc(136 * n)
    try:
        for g2, d_pts, prep, tables in ((False, d1, msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES),
                                        (True, d2, msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES)):
            pts = p2 if g2 else p1
            input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 0, 0, tables, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 0, 0, 0, tables, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 0, 0, 9, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 2, 0, 0, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 0, 3, 0, 0, g2=g2)
            input_error(cfg.mul_points_device, None, d_pts, n, d_out, 0, 0, 0, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, None, n, d_out, 0, 0, 0, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, n, None, 0, 0, 0, 0, g2=g2)
            input_error(cfg.mul_points_device, d_sc, d_pts, 1 << 32, d_out, 0, 0, 0, 0, g2=g2)
            input_error(cfg.mul_points, sc, pts, n, 0, 0, prep, 0, g2=g2)            # prepared on a host-buffer call
            input_error(cfg.mul_points, sc, pts, n, 0, 0, 0, prep, g2=g2)
            if not g2:
                input_error(cfg.mul_points_device, d_sc, d_pts, n, d_out, 0, 0, 0, msm_pkg.POINT_ARK_PROJECTIVE)
            cfg.mul_points_device(None, None, 0, None, 0, 0, 0, 0, g2=g2)            # n == 0: OK, nothing touched
            assert cfg.mul_points(None, None, 0, g2=g2) == b""
            size = 128 if g2 else 64
            cfg.mul_points_device(d_sc, d_pts, n, d_out, 0, 0, 0, 0, g2=g2)          # the ctx is as good as before
            assert cfg.to_host(d_out, size * n) == bytes(size * n)                   # zero scalars: identities
    finally:
        for p in (d_sc, d1, d2, d_out):
            cfg.free(p)


def test_mul_behind_a_held_stream_times_out_and_recovers(msm_pkg):
    n = 40
    ks, _, _ = case(msm_pkg, 1)
    sc = m.scalars_bytes(ks[:n], 0)
    b1, b2 = m.base_record(1, 0, o.GEN), m.base_record(2, 0, g.GEN2)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)
        for base, is_g2, name in ((b1, False, "msm_amd_mul_points"), (b2, True, "msm_amd_g2_mul_points")):
            with pytest.raises(msm_pkg.MsmError) as e:
                c2.mul_points(sc, base, n, m.ONE, g2=is_g2)
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.mul_points(sc, b1, n, m.ONE) == msm_pkg.host_mul_points(sc, b1, n, m.ONE)
        assert c2.mul_points(sc, b2, n, m.ONE, g2=True) == msm_pkg.host_mul_points(sc, b2, n, m.ONE, g2=True)
    finally:
        c2.close()


# ---- 9. the model at every position -------------------------------------------------------------------------------------------------
def assert_all(got, group, lo, exp, names=None):
    hst.assert_same(got, hst.encoded(group, lo, exp), group, lo, names)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [257, 4099])
def test_scalar_progression_one_base(cfg, msm_pkg, group, n):
    ks, base, exp = m.scalar_progression(group, 4099)
    lo = m.OUT_LAYOUTS[group][n % 2]
    assert_all(everywhere(cfg, msm_pkg, group, m.ONE, ks[:n], [base] * n, lo=lo), group, lo, exp[:n])


@pytest.mark.parametrize("group", GROUPS)
def test_whole_table_and_digit_edges(cfg, msm_pkg, group):
    plan = msm_pkg.mul_plan(group)
    ks, names, base, exp = m.table_case(group, plan["c"], plan["W"])
    assert_all(everywhere(cfg, msm_pkg, group, m.ONE, ks, [base] * len(ks), sl=1), group, 0, exp, names)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("which", ["random", "r - 1"])
def test_base_progression_each(cfg, msm_pkg, group, which):
    s = m.R - 1 if which == "r - 1" else random.Random(808).randrange(m.R)
    bases, exp = m.base_progression(group, s, 257)
    assert_all(everywhere(cfg, msm_pkg, group, m.EACH, [s] * 257, bases, sl=2), group, 0, exp)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_star_scalar_doubles_in_the_last_addition(cfg, msm_pkg, group, mode):
    """s* = 96 2^248 - r, s* +- 1, s* + r, s* + 4 r on three bases (mul_ref.S_STAR)"""
    stored, ks = m.star_scalars()
    for base, layouts in m.star_bases(group):
        exp = [m.expected(group, k, base) for k in ks]
        for sl in layouts:                                    # the Montgomery layout stores the reduced scalar
            assert_all(everywhere(cfg, msm_pkg, group, mode, stored if sl else ks, [base] * len(ks), sl=sl), group, 0, exp)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("y", m.ORDER3_Y)
def test_g1_base_of_order_3(cfg, msm_pkg, mode, y):
    """The G1 base (0, y) of order 3: doubling, vanishing sum and identity table entries on G1.  Pins the branch
    behaviour of the additions, not an API promise: the header leaves bases off the curve unspecified."""
    ks, bases, exp = hst.order3_case(mode, y)
    got = everywhere(cfg, msm_pkg, 1, mode, ks, bases)
    assert_all(got, 1, 0, exp)
    for i, k in enumerate(ks):
        assert (got[64 * i:64 * i + 64] == bytes(64)) == (k % 3 == 0), i


# ---- 10. resources ---------------------------------------------------------------------------------------------------------------------------
def test_mul_kernels_use_no_scratch():
    hst.test_mul_kernels_use_no_scratch()
