"""GPU tests of the BN254 G2 MSM: the device G2 arithmetic bit-exact with its host twin, msm_g2 / msm_g2_device against
the CPU G2 MSM and the big-integer model, every window size, discrete-log identities up to 2^20 points, adversarial
bucket distributions, and G1 results of the same ctx unchanged by G2 calls."""
import random

import pytest

import g2_ref as g
import test_g2_host as th

pytestmark = pytest.mark.gpu

SCALAR_CANON_LE = 1


# ---- device arithmetic == host twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1])
def test_device_fq2_ops_match_host(cfg, msm_pkg, op):
    cases = th.fq2_corpus(10 + op)
    a = [w for x, _ in cases for w in g.pad(x)]
    b = [w for _, y in cases for w in g.pad(y)]
    dev = cfg.test_op_g2(op, a, b, len(cases))
    assert dev == msm_pkg.test_op_g2_host(op, a, b, len(cases))
    for i, (x, y) in enumerate(cases):
        th.check_fq2(op, x, y, dev[80 * i:80 * i + 80])


@pytest.mark.parametrize("op", th.POINT_OPS)
def test_device_point_ops_match_host(cfg, msm_pkg, op):
    cases = th.point_corpus(op, 50 + op)
    a = [w for c in cases for w in c[0]]
    b = [w for c in cases for w in c[1]]
    dev = cfg.test_op_g2(op, a, b, len(cases))
    assert dev == msm_pkg.test_op_g2_host(op, a, b, len(cases))
    for i, (_, _, exp, van) in enumerate(cases):
        th.check_point(dev[80 * i:80 * i + 80], exp, van)


# ---- small MSMs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 257])
def test_msm_g2_small_cases(cfg, msm_pkg, n):
    ks, dl = th.msm_case(n, 1000 + n)
    exp = th.expected(ks, dl)
    for sl, pl in ((0, 0), (1, 1), (2, 0)):
        sc, pts = th.encode_case(ks, dl, sl, pl)
        out = cfg.msm_g2(sc, pts, n, scalar_layout=sl, point_layout=pl)
        th.assert_result(out, exp)
        assert out == msm_pkg.host_msm_g2(sc, pts, n, threads=4, scalar_layout=sl, point_layout=pl)
        ds, dp = cfg.alloc(len(sc)), cfg.alloc(len(pts))
        try:
            cfg.to_device(ds, sc)
            cfg.to_device(dp, pts)
            assert cfg.msm_g2_device(ds, dp, n, scalar_layout=sl, point_layout=pl) == out
        finally:
            cfg.free(ds)
            cfg.free(dp)


def test_msm_g2_empty_and_errors(cfg, msm_pkg):
    assert cfg.msm_g2(b"", b"", 0) == g.identity_bytes()
    with pytest.raises(msm_pkg.MsmError) as e:
        cfg.msm_g2(bytes(32), bytes(128), 1, point_layout=5)
    assert e.value.status == msm_pkg.INPUT_ERROR
    out = bytes(192)
    assert msm_pkg.lib().msm_amd_msm_g2(cfg.h, 0, 0, None, None, 4, out) == msm_pkg.INPUT_ERROR


# ---- progressions: window sizes and discrete-log identities ---------------------------------------------------------
def progression_instance(msm_pkg, n, a0, d, seed):
    """bases P_i = (a0 + i d) G2 (library progression generator), canonical scalars k_i < r, and the expected
    (sum k_i (a0 + i d)) G2 from big integers and one scalar multiplication"""
    import numpy as np
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(a0, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    words[:, 7] &= 0x0FFFFFFF   # < 2^252 < r
    sc = words.tobytes()
    q = np.frombuffer(sc, dtype="<u2").reshape(n, 16).astype(np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    sum_k = sum(int(v) << (16 * j) for j, v in enumerate(q.sum(axis=0)))
    sum_ik = sum(int(v) << (16 * j) for j, v in enumerate((q * idx[:, None]).sum(axis=0)))
    s = (a0 * sum_k + d * sum_ik) % g.R_ORDER
    return sc, pts, g.scalar_mul(s, g.GEN2)


def test_msm_g2_every_window_size(cfg, msm_pkg):
    n = 1 << 12
    sc, pts, exp = progression_instance(msm_pkg, n, 1234567, 7654321, 5)
    ref = msm_pkg.host_msm_g2(sc, pts, n, threads=8, scalar_layout=SCALAR_CANON_LE)
    th.assert_result(ref, exp)
    try:
        for c in range(3, 18):
            cfg.set_window_size(c)
            assert cfg.msm_g2(sc, pts, n, scalar_layout=SCALAR_CANON_LE) == ref, c
    finally:
        cfg.set_window_size(0)


@pytest.mark.parametrize("logn", [16, 18, 20])
def test_msm_g2_dlog_identity(cfg, msm_pkg, logn):
    n = 1 << logn
    sc, pts, exp = progression_instance(msm_pkg, n, 0xC0FFEE + logn, 0xBEEF + 3 * logn, logn)
    ds, dp = cfg.alloc(len(sc)), cfg.alloc(len(pts))
    try:
        cfg.to_device(ds, sc)
        cfg.to_device(dp, pts)
        th.assert_result(cfg.msm_g2_device(ds, dp, n, scalar_layout=SCALAR_CANON_LE), exp)
    finally:
        cfg.free(ds)
        cfg.free(dp)


# ---- adversarial bucket distributions -------------------------------------------------------------------------------
def test_msm_g2_all_scalars_equal(cfg, msm_pkg):
    """one bucket per window holds every point: split into many work items, summed by the combine kernels"""
    n = 1 << 14
    d = 99991
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(d, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    k = 0x1234567890ABCDEF1234567890ABCDEF
    sc = g.encode_scalar(k, 1) * n
    exp = g.scalar_mul(k * d * (n * (n + 1) // 2) % g.R_ORDER, g.GEN2)
    for c in (0, 8, 16):
        cfg.set_window_size(c)
        try:
            th.assert_result(cfg.msm_g2(sc, pts, n, scalar_layout=1), exp)
        finally:
            cfg.set_window_size(0)


def test_msm_g2_opposite_halves_and_duplicates(cfg, msm_pkg):
    rng = random.Random(11)
    n = 1 << 12
    p = g.scalar_mul(31337, g.GEN2)
    ks = [rng.randrange(g.R_ORDER) for _ in range(n // 2)]
    # half P, half -P with the same scalars: everything cancels
    pts = g.encode_h2c(p) * (n // 2) + g.encode_h2c(g.neg(p)) * (n // 2)
    sc = b"".join(g.encode_scalar(k, 0) for k in ks) * 2
    assert cfg.msm_g2(sc, pts, n) == g.identity_bytes()
    # many duplicates: 8 distinct bases, each repeated n / 8 times, small scalars (shared buckets)
    bases = [g.scalar_mul(1000 + 17 * j, g.GEN2) for j in range(8)]
    ks = [rng.randrange(1, 64) for _ in range(n)]
    pts = b"".join(g.encode_h2c(bases[i % 8]) for i in range(n))
    sc = b"".join(g.encode_scalar(k, 0) for k in ks)
    s = sum(k * (1000 + 17 * (i % 8)) for i, k in enumerate(ks)) % g.R_ORDER
    out = cfg.msm_g2(sc, pts, n)
    th.assert_result(out, g.scalar_mul(s, g.GEN2))
    assert out == msm_pkg.host_msm_g2(sc, pts, n, threads=8)


def test_g1_unchanged_by_g2_calls(cfg, msm_pkg):
    from oracle import bn254_ref as o
    from oracle import c_oracle as co
    n = 1 << 12
    points, scalars = co.gen_instance(o.SEED_BASE + 7, n)
    before = cfg.msm(scalars, points, n)
    ks, dl = th.msm_case(64, 3)
    sc, pts = th.encode_case(ks, dl, 0, 0)
    g2_before = cfg.msm_g2(sc, pts, 64)
    dp, ds = cfg.generate_instance(o.SEED_BASE + 9, 1 << 16, True)
    try:
        dev_before = cfg.msm_batch_device([ds], [dp], [1 << 16])[0]
        sc2, pts2, _ = progression_instance(msm_pkg, 1 << 16, 5, 7, 1)
        cfg.msm_g2(sc2, pts2, 1 << 16, scalar_layout=1)
        assert cfg.msm(scalars, points, n) == before
        assert cfg.msm_batch_device([ds], [dp], [1 << 16])[0] == dev_before
        assert cfg.msm_g2(sc, pts, 64) == g2_before
    finally:
        cfg.free(dp)
        cfg.free(ds)


# ---- one instance body for G1 and G2: the G2 call in its own workspace and slot ---------------------------------------
def _g1_on_device(cfg, seed, n):
    """(d_scalars, d_points, the C oracle's result as a canonical affine point) of a generated G1 instance"""
    from oracle import bn254_ref as o
    from oracle import c_oracle as co
    points, scalars = co.gen_instance(seed, n)
    ds, dp = cfg.alloc(len(scalars)), cfg.alloc(len(points))
    cfg.to_device(ds, scalars)
    cfg.to_device(dp, points)
    return ds, dp, o.decode_jacobian_mont_le(co.msm_best(scalars, points, n, 2))


def _assert_g1(out, exp):
    from oracle import bn254_ref as o
    assert o.decode_jacobian_mont_le(out) == exp


def test_g2_between_g1_submit_and_wait(cfg, msm_pkg):
    """a G2 MSM while a G1 batch of the same ctx is between submit and wait: the G2 call runs in its own workspace and
    slot, so neither disturbs the other"""
    from oracle import bn254_ref as o
    n1, n2 = 1 << 10, 1 << 8
    sc2, pts2, exp2 = progression_instance(msm_pkg, n2, 0xABCDE, 0x1357, 8)
    g1 = [_g1_on_device(cfg, o.SEED_BASE + 30 + i, n1) for i in range(2)]
    try:
        h = cfg.submit_batch_device([i[0] for i in g1], [i[1] for i in g1], [n1, n1])
        out2 = cfg.msm_g2(sc2, pts2, n2, scalar_layout=SCALAR_CANON_LE)
        outs = cfg.wait_batch(h)
        th.assert_result(out2, exp2)
        assert out2 == msm_pkg.host_msm_g2(sc2, pts2, n2, threads=4, scalar_layout=SCALAR_CANON_LE)
        for out, inst in zip(outs, g1):
            _assert_g1(out, inst[2])
    finally:
        for ds, dp, _ in g1:
            cfg.free(ds)
            cfg.free(dp)


def test_g2_timings_mean_what_g1_timings_mean(cfg, msm_pkg):
    """msm_amd_last_timings after a G2 call whose combine pass runs (equal scalars: every window has one bucket of 2^8
    points, cut into items of CH = 16): the accumulate fields are the accumulate kernel alone, the total is the sum of
    the stage spans and reserved2[0] the work items, as for a G1 instance"""
    n = 1 << 8
    d = 4242
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(d, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    k = 0x0FEDCBA987654321FEDCBA9876543210F
    out = cfg.msm_g2(g.encode_scalar(k, 1) * n, pts, n, scalar_layout=SCALAR_CANON_LE)
    t = cfg.timings()
    p = cfg.test_g2_last_plan()
    th.assert_result(out, g.scalar_mul(k * d * (n * (n + 1) // 2) % g.R_ORDER, g.GEN2))
    assert p["CH"] == 16 and p["multi_count"] > 0, p   # the combine pass had work
    assert (t.n, t.window_size, t.num_windows) == (p["n_scalars"], p["c"], p["W_digits"])
    assert t.n == n
    assert t.reserved == 1
    assert t.reserved2[0] == p["total_items"]
    assert t.accumulate_kernel_ms == t.accumulate_ms
    stages = (t.convert_ms, t.digits_ms, t.sort_ms, t.accumulate_ms, t.reduce_ms)
    print("G2 timings:", stages, t.total_gpu_ms)
    assert all(s > 0.0 for s in stages[1:]), stages
    assert t.total_gpu_ms == pytest.approx(sum(stages), rel=1e-6)   # a float sum of five floats


def test_g2_slot_reuse_across_sizes_and_groups(msm_pkg):
    """2^6, 2^10 and 2^6 points again through one ctx (the G2 slot and workspace grow, then hold a smaller instance), a
    lone G1 call in between: every result exact, and after every G2 call the plan tap reads what a fresh ctx reads"""
    from oracle import bn254_ref as o
    COUNTERS = ("total_items", "multi_count", "deferred")
    small = progression_instance(msm_pkg, 1 << 6, 77, 5, 6)
    big = progression_instance(msm_pkg, 1 << 10, 99, 3, 10)
    ctx = msm_pkg.MsmConfig(0)
    try:
        def g2_call(c, inst):
            sc, pts, exp = inst
            n = len(sc) // 32
            out = c.msm_g2(sc, pts, n, scalar_layout=SCALAR_CANON_LE)
            th.assert_result(out, exp)
            assert out == msm_pkg.host_msm_g2(sc, pts, n, threads=4, scalar_layout=SCALAR_CANON_LE)
            return c.test_g2_last_plan()

        fresh = {}
        for name, inst in (("small", small), ("big", big)):
            f = msm_pkg.MsmConfig(0)
            try:
                fresh[name] = g2_call(f, inst)
            finally:
                f.close()
        assert fresh["small"]["total_items"] != fresh["big"]["total_items"]
        n1 = 1 << 10
        ds, dp, exp1 = _g1_on_device(ctx, o.SEED_BASE + 40, n1)
        try:
            for name, inst in (("small", small), ("big", big), ("small", small)):
                p = g2_call(ctx, inst)
                assert p == fresh[name], (name, {k: (p[k], fresh[name][k]) for k in COUNTERS})
                _assert_g1(ctx.msm_batch_device([ds], [dp], [n1])[0], exp1)
                assert ctx.test_last_plan()["lone"] == 1
                assert ctx.test_g2_last_plan() == fresh[name]   # the G1 call left the G2 slot alone
        finally:
            ctx.free(ds)
            ctx.free(dp)
    finally:
        ctx.close()
