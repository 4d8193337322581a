"""GPU tests of the persistent G2 bases and the precomputed G2 window tables: the new device arithmetic bit-exact with
its host twin, the table build against the host twin, the prepared and the table paths byte for byte against the
per-call G2 MSM and against the big-integer model, discrete-log identities up to 2^20 points, argument errors, handle
lifetime, and G1 / per-call G2 results of the same ctx unchanged."""
import random

import pytest

import g2_ref as g
import test_g2_host as th
import test_g2_tables_host as tt

pytestmark = pytest.mark.gpu

CANON = 1   # MSM_AMD_SCALAR_CANON_LE
WINDOWS = [4, 9, 15, 16, 18, 21, 0]   # 0 = automatic; u16 digits up to 15, u32 above


def le(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


def on_device(cfg, data):
    d = cfg.alloc(len(data))
    cfg.to_device(d, data)
    return d


def progression(msm_pkg, n, a0, d, idents=()):
    """bases P_i = (a0 + i d) G2 from the library's generator, identities at `idents`; (points bytes, discrete logs)"""
    pts = bytearray(msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(a0, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n))
    dl = [a0 + i * d for i in range(n)]
    for i in idents:
        pts[128 * i:128 * i + 128] = bytes(128)
        dl[i] = 0
    return bytes(pts), dl


def expected(ks, dl):
    return g.scalar_mul(sum(k * a for k, a in zip(ks, dl)) % g.R_ORDER, g.GEN2)


def progression_instance(msm_pkg, n, a0, d, seed):
    """the discrete-log identity of the per-call G2 tests: bases (a0 + i d) G2, canonical scalars k_i < 2^252, and
    (sum k_i (a0 + i d)) G2 from big integers and one scalar multiplication"""
    import numpy as np
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(a0, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    words[:, 7] &= 0x0FFFFFFF
    sc = words.tobytes()
    q = np.frombuffer(sc, dtype="<u2").reshape(n, 16).astype(np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    sum_k = sum(int(v) << (16 * j) for j, v in enumerate(q.sum(axis=0)))
    sum_ik = sum(int(v) << (16 * j) for j, v in enumerate((q * idx[:, None]).sum(axis=0)))
    return sc, pts, g.scalar_mul((a0 * sum_k + d * sum_ik) % g.R_ORDER, g.GEN2)


# ---- 4. new raw ops: device == host twin ------------------------------------------------------------------------------
def test_device_fq2_inv_matches_host(cfg, msm_pkg):
    cases = tt.inv_corpus(21)
    a = [w for x in cases for w in g.pad(x)]
    dev = cfg.test_op_g2(msm_pkg.G2_RAW_FQ2_INV, a, [0] * len(a), len(cases))
    assert dev == msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_FQ2_INV, a, [0] * len(a), len(cases))
    for i, x in enumerate(cases):
        tt.check_inv(x, dev[80 * i:80 * i + 80])


def test_device_pt_to_affine_matches_host(cfg, msm_pkg):
    cases = tt.affine_corpus(22)
    a = [w for c in cases for w in c[0]]
    dev = cfg.test_op_g2(msm_pkg.G2_RAW_PT_TO_AFFINE, a, [0] * len(a), len(cases))
    assert dev == msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_PT_TO_AFFINE, a, [0] * len(a), len(cases))
    for i, (w, pt) in enumerate(cases):
        tt.check_affine(w, dev[80 * i:80 * i + 80], pt)


# ---- 5. the table build == its host twin ------------------------------------------------------------------------------
def read_whole_table(cfg, t, n, W):
    return b"".join(cfg.g2_tables_read(t, w, 0, n) for w in range(W))


@pytest.mark.parametrize("c", [4, 7, 16, 21])
def test_tables_read_equals_host_twin(cfg, msm_pkg, c):
    n = 257
    pts, _ = progression(msm_pkg, n, 4242 + c, 977, idents=(0, 100, 256))
    ark = b"".join(pts[128 * i:128 * i + 128] + (b"\x01" if i in (0, 100, 256) else b"\x00") + bytes(7) for i in range(n))
    W = 254 // c + 1
    want = msm_pkg.g2_table_host(pts, n, c, W, threads=8)
    for buf, layout in ((pts, 0), (ark, 1)):
        t = cfg.g2_tables_build(buf, n, point_layout=layout, window_size=c)
        try:
            info = cfg.g2_tables_info(t)
            assert info == {"n": n, "window_size": c, "num_windows": W, "device_bytes": 128 * n * W}
            assert read_whole_table(cfg, t, n, W) == want
            assert cfg.g2_tables_read(t, W - 1, 100, 1) == bytes(128)          # the identity stays the identity
            assert cfg.g2_tables_read(t, 1, 5, 7) == want[128 * (n + 5):128 * (n + 12)]
        finally:
            cfg.g2_tables_free(t)


def test_tables_read_equals_host_twin_auto_window(cfg, msm_pkg):
    n = 1 << 12
    pts, _ = progression(msm_pkg, n, 31, 17, idents=(9,))
    dp = on_device(cfg, pts)
    t = cfg.g2_tables_build_device(dp, n)
    try:
        info = cfg.g2_tables_info(t)
        c, W = info["window_size"], info["num_windows"]
        assert 4 <= c <= 21 and W == 254 // c + 1 and info["device_bytes"] == 128 * n * W
        assert read_whole_table(cfg, t, n, W) == msm_pkg.g2_table_host(pts, n, c, W, threads=16)
    finally:
        cfg.g2_tables_free(t)
        cfg.free(dp)


# ---- 6. prepared bases ------------------------------------------------------------------------------------------------
def check_prepared(cfg, msm_pkg, n, cases):
    """cases: [(scalar layout, point layout, scalars, points)] of ONE instance; every way to the prepared path gives the
    bytes of msm_g2 on the same inputs"""
    for sl, pl, sc, pts, exp in cases:
        ref = cfg.msm_g2(sc, pts, n, scalar_layout=sl, point_layout=pl)
        th.assert_result(ref, exp)
        d_up = cfg.g2_bases_upload(pts, n, point_layout=pl)
        dp = on_device(cfg, pts)
        ds = on_device(cfg, sc)
        d_pr = cfg.g2_bases_prepare_device(dp, n, point_layout=pl)
        try:
            assert cfg.to_host(d_up, 128 * n) == cfg.to_host(d_pr, 128 * n)
            for d in (d_up, d_pr):
                assert cfg.msm_g2_prepared(sc, d, n, scalar_layout=sl) == ref, (n, sl, pl)
                assert cfg.msm_g2_device(ds, d, n, scalar_layout=sl, point_layout=msm_pkg.G2_POINT_PREPARED) == ref
            t = cfg.timings()
            assert t.n == n and t.num_windows == 254 // t.window_size + 1
        finally:
            for d in (d_up, d_pr, dp, ds):
                cfg.free(d)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 257])
def test_prepared_path_small_cases(cfg, msm_pkg, n):
    ks, dl = th.msm_case(n, 2000 + n)
    exp = th.expected(ks, dl)
    cases = []
    for sl in (0, 1, 2):
        for pl in (0, 1):
            sc, pts = th.encode_case(ks, dl, sl, pl)
            cases.append((sl, pl, sc, pts, exp))
    check_prepared(cfg, msm_pkg, n, cases)


def test_prepared_path_4096(cfg, msm_pkg):
    n = 4096
    rng = random.Random(4096)
    idents = (1, 9, 4095)
    pts, dl = progression(msm_pkg, n, 555, 333, idents=idents)
    ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
    ks[0], ks[2] = g.R_ORDER - 1, 0
    exp = expected(ks, dl)
    ark = b"".join(pts[128 * i:128 * i + 128] + (b"\x01" if i in idents else b"\x00") + bytes(7) for i in range(n))
    cases = [(sl, pl, b"".join(g.encode_scalar(k, sl) for k in ks), buf, exp)
             for sl in (0, 1, 2) for pl, buf in ((0, pts), (1, ark))]
    check_prepared(cfg, msm_pkg, n, cases)


# ---- 7. the table path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 4096, 1 << 16])
def test_table_path_equals_per_call(cfg, msm_pkg, n):
    rng = random.Random(n)
    pts, dl = progression(msm_pkg, n, 1000003, 7919, idents=(3, n - 1))
    ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
    ks[0], ks[1], ks[2] = g.R_ORDER - 1, (1 << 253) - 1, 0
    sc = le(ks)
    ks2 = [(3 * k + 5) % g.R_ORDER for k in ks]
    sc2 = le(ks2)
    ref, ref2 = cfg.msm_g2(sc, pts, n, scalar_layout=CANON), cfg.msm_g2(sc2, pts, n, scalar_layout=CANON)
    th.assert_result(ref, expected(ks, dl))
    th.assert_result(ref2, expected(ks2, dl))
    mont = b"".join(g.encode_scalar(k, 0) for k in ks) if n <= 4096 else None
    ds2 = on_device(cfg, sc2)
    try:
        for c in WINDOWS:
            t = cfg.g2_tables_build(pts, n, window_size=c)
            try:
                info = cfg.g2_tables_info(t)
                assert info["n"] == n and (c == 0 or info["window_size"] == c)
                assert cfg.msm_g2_tables(sc, t, scalar_layout=CANON) == ref, (n, c)
                tm = cfg.timings()
                assert (tm.n, tm.window_size, tm.num_windows) == (n, info["window_size"], info["num_windows"])
                assert cfg.msm_g2_device(ds2, t, n, scalar_layout=CANON, point_layout=msm_pkg.G2_POINT_TABLES) == ref2, (n, c)
                if mont:
                    assert cfg.msm_g2_tables(mont, t) == ref, (n, c)
            finally:
                cfg.g2_tables_free(t)
    finally:
        cfg.free(ds2)


@pytest.mark.parametrize("c", WINDOWS)
def test_table_path_scalar_edge_cases(cfg, msm_pkg, c):
    """0, 1, r - 1, 2^253 and, for several windows w, 2^(c w) - 1 (all lower digits at their maximum) and 2^(c w - 1)
    (the digit that turns negative and carries) -- up to the top window -- against the big-integer model"""
    n = 50
    rng = random.Random(77 + c)
    pts, dl = progression(msm_pkg, n, 123457, 1009, idents=(4,))
    t = cfg.g2_tables_build(pts, n, window_size=c)
    try:
        info = cfg.g2_tables_info(t)
        cc, W = info["window_size"], info["num_windows"]
        ks = [0, 1, g.R_ORDER - 1, 1 << 253, g.R_ORDER - 2]
        for w in sorted({1, 2, W // 2, W - 2, W - 1}):
            ks += [(1 << (cc * w)) - 1, 1 << (cc * w - 1), (1 << (cc * w)) + (1 << (cc * w - 1))]
        assert len(ks) <= n and all(k < g.R_ORDER for k in ks)
        ks += [rng.randrange(g.R_ORDER) for _ in range(n - len(ks))]
        rng.shuffle(ks)
        exp = expected(ks, dl)
        for sl in (0, 1, 2):
            sc = b"".join(g.encode_scalar(k, sl) for k in ks)
            out = cfg.msm_g2_tables(sc, t, scalar_layout=sl)
            th.assert_result(out, exp)
            assert out == cfg.msm_g2(sc, pts, n, scalar_layout=sl)
            ds = on_device(cfg, sc)
            try:
                assert cfg.msm_g2_device(ds, t, n, scalar_layout=sl, point_layout=msm_pkg.G2_POINT_TABLES) == out
            finally:
                cfg.free(ds)
    finally:
        cfg.g2_tables_free(t)


def test_table_path_all_scalars_equal(cfg, msm_pkg):
    """every entry of a digit window falls into one slot: split buckets, both combine kernels"""
    n = 1 << 14
    d = 99991
    pts, _ = progression(msm_pkg, n, d, d)
    k = 0x1234567890ABCDEF1234567890ABCDEF
    sc = g.encode_scalar(k, CANON) * n
    exp = g.scalar_mul(k * d * (n * (n + 1) // 2) % g.R_ORDER, g.GEN2)
    ref = cfg.msm_g2(sc, pts, n, scalar_layout=CANON)
    th.assert_result(ref, exp)
    for c in (0, 8, 16):
        t = cfg.g2_tables_build(pts, n, window_size=c)
        try:
            assert cfg.msm_g2_tables(sc, t, scalar_layout=CANON) == ref, c
        finally:
            cfg.g2_tables_free(t)
    d_prep = cfg.g2_bases_upload(pts, n)
    try:
        assert cfg.msm_g2_prepared(sc, d_prep, n, scalar_layout=CANON) == ref
    finally:
        cfg.free(d_prep)


def test_table_path_opposite_halves_cancel(cfg, msm_pkg):
    rng = random.Random(11)
    n = 1 << 12
    p = g.scalar_mul(31337, g.GEN2)
    pts = g.encode_h2c(p) * (n // 2) + g.encode_h2c(g.neg(p)) * (n // 2)
    sc = b"".join(g.encode_scalar(rng.randrange(g.R_ORDER), 0) for _ in range(n // 2)) * 2
    for c in (0, 16):
        t = cfg.g2_tables_build(pts, n, window_size=c)
        try:
            assert cfg.msm_g2_tables(sc, t) == g.identity_bytes()
        finally:
            cfg.g2_tables_free(t)
    d_prep = cfg.g2_bases_upload(pts, n)
    try:
        assert cfg.msm_g2_prepared(sc, d_prep, n) == g.identity_bytes()
    finally:
        cfg.free(d_prep)


# ---- 8. discrete-log identities at 2^18 and 2^20 ----------------------------------------------------------------------
def test_dlog_identity_2p18_tables(cfg, msm_pkg):
    n = 1 << 18
    sc, pts, exp = progression_instance(msm_pkg, n, 0xC0FFEE + 18, 0xBEEF + 54, 18)
    t = cfg.g2_tables_build(pts, n)
    try:
        out = cfg.msm_g2_tables(sc, t, scalar_layout=CANON)
        th.assert_result(out, exp)
        assert out == cfg.msm_g2(sc, pts, n, scalar_layout=CANON)
    finally:
        cfg.g2_tables_free(t)


@pytest.fixture(scope="module")
def big(cfg, msm_pkg):
    """the 2^20 instance: device-resident scalars and points, ONE table (automatic window) and one prepared array"""
    n = 1 << 20
    sc, pts, exp = progression_instance(msm_pkg, n, 0xC0FFEE + 20, 0xBEEF + 60, 20)
    ds, dp = on_device(cfg, sc), on_device(cfg, pts)
    t = cfg.g2_tables_build_device(dp, n)
    d_prep = cfg.g2_bases_prepare_device(dp, n)
    yield {"n": n, "ds": ds, "dp": dp, "tables": t, "prepared": d_prep, "exp": exp, "sc": sc}
    cfg.g2_tables_free(t)
    for d in (ds, dp, d_prep):
        cfg.free(d)


def test_dlog_identity_2p20_tables(cfg, msm_pkg, big):
    info = cfg.g2_tables_info(big["tables"])
    assert info["n"] == big["n"] and info["device_bytes"] == 128 * big["n"] * info["num_windows"]
    out = cfg.msm_g2_device(big["ds"], big["tables"], big["n"], scalar_layout=CANON, point_layout=msm_pkg.G2_POINT_TABLES)
    th.assert_result(out, big["exp"])
    assert cfg.msm_g2_tables(big["sc"], big["tables"], scalar_layout=CANON) == out
    assert cfg.msm_g2_device(big["ds"], big["dp"], big["n"], scalar_layout=CANON) == out


def test_dlog_identity_2p20_prepared(cfg, msm_pkg, big):
    out = cfg.msm_g2_device(big["ds"], big["prepared"], big["n"], scalar_layout=CANON,
                            point_layout=msm_pkg.G2_POINT_PREPARED)
    th.assert_result(out, big["exp"])
    assert cfg.msm_g2_prepared(big["sc"], big["prepared"], big["n"], scalar_layout=CANON) == out


# ---- 9. errors and lifetime -------------------------------------------------------------------------------------------
def input_error(msm_pkg, fn, *a, **kw):
    with pytest.raises(msm_pkg.MsmError) as e:
        fn(*a, **kw)
    assert e.value.status == msm_pkg.INPUT_ERROR, e.value


def test_table_and_prepared_errors(cfg, msm_pkg):
    from oracle import bn254_ref as o
    from oracle import c_oracle as co
    n = 50
    pts, dl = progression(msm_pkg, n, 5, 7)
    sc = le([random.Random(1).randrange(g.R_ORDER) for _ in range(n)])
    for c in (3, 22, 1, 255):
        input_error(msm_pkg, cfg.g2_tables_build, pts, n, window_size=c)
    for layout in (2, 3, 5, 7):   # tables and prepared arrays come from the two host layouts only
        input_error(msm_pkg, cfg.g2_tables_build, pts, n, point_layout=layout)
        input_error(msm_pkg, cfg.g2_bases_upload, pts, n, point_layout=layout)
        input_error(msm_pkg, cfg.msm_g2, sc, pts, n, scalar_layout=CANON, point_layout=layout)   # host buffers
    ds, dp = on_device(cfg, sc), on_device(cfg, pts)
    g1_pts, g1_sc = co.gen_instance(o.SEED_BASE + 3, n)
    d_g1sc = on_device(cfg, g1_sc)
    t = cfg.g2_tables_build(pts, n)
    g1t = cfg.tables_build(g1_pts, n)
    TAB = msm_pkg.G2_POINT_TABLES
    try:
        ref = cfg.msm_g2_device(ds, t, n, scalar_layout=CANON, point_layout=TAB)
        assert ref == cfg.msm_g2(sc, pts, n, scalar_layout=CANON)
        input_error(msm_pkg, cfg.msm_g2_device, ds, t, n - 1, scalar_layout=CANON, point_layout=TAB)     # n mismatch
        input_error(msm_pkg, cfg.msm_g2_device, ds, t, 0, scalar_layout=CANON, point_layout=TAB)
        input_error(msm_pkg, cfg.msm_g2_device, ds, dp, n, scalar_layout=CANON, point_layout=TAB)        # no handle
        input_error(msm_pkg, cfg.msm_g2_device, ds, g1t, n, scalar_layout=CANON, point_layout=TAB)       # a G1 handle
        input_error(msm_pkg, cfg.msm_g2_tables, sc, g1t, scalar_layout=CANON)
        input_error(msm_pkg, cfg.g2_tables_info, g1t)
        input_error(msm_pkg, cfg.g2_tables_free, g1t)
        input_error(msm_pkg, cfg.g2_tables_read, g1t, 0, 0, 1)
        input_error(msm_pkg, cfg.msm_batch_device, [d_g1sc], [t], [n], point_layout=msm_pkg.POINT_TABLES)   # G2 handle, G1 call
        input_error(msm_pkg, cfg.tables_info, t)
        input_error(msm_pkg, cfg.tables_free, t)
        input_error(msm_pkg, cfg.msm_g2_tables, sc, t, scalar_layout=9)
        input_error(msm_pkg, cfg.g2_tables_read, t, cfg.g2_tables_info(t)["num_windows"], 0, 1)
        input_error(msm_pkg, cfg.g2_tables_read, t, 0, n - 1, 2)
        assert cfg.msm_g2_device(ds, t, n, scalar_layout=CANON, point_layout=TAB) == ref   # both handles still good
        assert cfg.msm_batch_device([d_g1sc], [g1t], [n], point_layout=msm_pkg.POINT_TABLES)[0] == cfg.msm(g1_sc, g1_pts, n)
    finally:
        cfg.tables_free(g1t)
        cfg.g2_tables_free(t)
        for d in (ds, dp, d_g1sc):
            cfg.free(d)
    input_error(msm_pkg, cfg.g2_tables_free, t)                                           # free twice
    input_error(msm_pkg, cfg.msm_g2_tables, sc, t, scalar_layout=CANON)                   # a freed handle


def test_table_freed_on_a_busy_ctx_and_destroy_with_a_live_table(msm_pkg):
    n = 300
    pts, dl = progression(msm_pkg, n, 11, 13, idents=(2,))
    rng = random.Random(5)
    ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
    sc = le(ks)
    c2 = msm_pkg.setup_metal_state()
    try:
        t = c2.g2_tables_build(pts, n, window_size=9)
        ref = c2.msm_g2_tables(sc, t, scalar_layout=CANON)
        th.assert_result(ref, expected(ks, dl))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)
        c2.g2_tables_free(t)              # the ctx is busy: the table memory goes to the graveyard, the call returns
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        input_error(msm_pkg, c2.msm_g2_tables, sc, t, scalar_layout=CANON)
        t2 = c2.g2_tables_build(pts, n, window_size=9)
        assert c2.msm_g2_tables(sc, t2, scalar_layout=CANON) == ref
        assert c2.msm_g2(sc, pts, n, scalar_layout=CANON) == ref
        c2.g2_tables_build(pts, n)        # two tables stay live: msm_amd_destroy releases them
    finally:
        c2.close()


# ---- 10. isolation ----------------------------------------------------------------------------------------------------
def test_g1_and_per_call_g2_unchanged_by_table_and_prepared_calls(cfg, msm_pkg):
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
        sc2, pts2, exp2 = progression_instance(msm_pkg, 1 << 16, 5, 7, 1)
        t = cfg.g2_tables_build(pts2, 1 << 16)
        d_prep = cfg.g2_bases_upload(pts2, 1 << 16)
        try:
            th.assert_result(cfg.msm_g2_tables(sc2, t, scalar_layout=CANON), exp2)
            th.assert_result(cfg.msm_g2_prepared(sc2, d_prep, 1 << 16, scalar_layout=CANON), exp2)
            assert cfg.msm(scalars, points, n) == before
            assert cfg.msm_batch_device([ds], [dp], [1 << 16])[0] == dev_before
            assert cfg.msm_g2(sc, pts, 64) == g2_before
        finally:
            cfg.g2_tables_free(t)
            cfg.free(d_prep)
        assert cfg.msm(scalars, points, n) == before
        assert cfg.msm_batch_device([ds], [dp], [1 << 16])[0] == dev_before
        assert cfg.msm_g2(sc, pts, 64) == g2_before
    finally:
        cfg.free(dp)
        cfg.free(ds)
