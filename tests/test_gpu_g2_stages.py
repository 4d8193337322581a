"""Stage tests of the G2 pipeline: digits, bucket sizes, every non-empty bucket, every window partial and the result of
a G2 MSM, read through the G2 stage tap (msm_amd_test_g2_last_plan / msm_amd_test_g2_stage_copy) after an ordinary
call and compared exactly with tests/g2_stage_ref.py (integer sums of known discrete logs, one fixed-base
multiplication per compared point):

  buckets     accumulate_g2_kernel, combine_small / combine_big (point_stages.hip.h on G2)
  partials    sum_groups / reduce_bits on G2, at the shapes of the level planner and of the thread picker
  classes     a replay of accumulate_g2_kernel's state machine on the tapped order counts which branch every step took
  poisoning   msm_amd_test_fill_workspaces before every call: no stale G2 bucket, partial or scratch point leaks"""
import ctypes
import random

import numpy as np
import pytest

import g2_ref as g
import g2_stage_ref as sr
import test_g2_host as th
import test_gpu_pipeline_stages as st

pytestmark = pytest.mark.gpu

CANON = 1   # MSM_AMD_SCALAR_CANON_LE
REDUCE_BITS_CAP = 128   # G2Stages::kReduceBitsThreads


def le(ks):
    return b"".join(int(k).to_bytes(32, "little") for k in ks)


@pytest.fixture(scope="module")
def bases():
    """512 bases with distinct discrete logs below 2^40, shared (and left unchanged) by the tests below"""
    dl = sr.distinct_dlogs(random.Random(2024), 512)
    return dl, sr.encode_points(dl)


def _u32(cfg, which):
    return np.frombuffer(cfg.test_g2_stage_copy(which), dtype=np.uint32)


def _tap_digits(cfg, msm_pkg, plan):
    raw = cfg.test_g2_stage_copy(msm_pkg.STAGE_DIGITS)
    dt, bits = (np.uint32, 32) if plan["wide_digits"] else (np.uint16, 16)
    v = np.frombuffer(raw, dtype=dt)
    d = (v & dt((1 << (bits - 1)) - 1)).astype(np.int32)
    np.negative(d, out=d, where=(v >> dt(bits - 1)) != 0)
    return d.reshape(plan["W_digits"], plan["n_scalars"])


def reduce_bits_threads(lb):
    """reduce_bits_threads of point_stages.hip.h for a lone call on G2"""
    t = 64
    while t < REDUCE_BITS_CAP and t < (1 << ((lb + 1) // 2)) // 2:
        t *= 2
    return t


def check_window_identity(parts, sums, lb):
    """partial[w][lb] + sum_k 2^k partial[w][k] == sum_s (s + 1) B[w][s], from the TAPPED partials (points)"""
    for w, wv in enumerate(sr.window_values(sums)):
        acc = parts[w * (lb + 1) + lb]
        for k in range(lb):
            acc = g.add(acc, g.scalar_mul(1 << k, parts[w * (lb + 1) + k]))
        assert acc == sr.point_of(wv), f"window {w}: weighted partials"


def check_g2_buckets(cfg, msm_pkg, ks, dlogs, out, c, counts=None, identity=False, tables=False):
    """The G2 twin of check_buckets: the tapped digits, the bucket sizes, every bucket with size != 0, every window
    partial and the result of the last G2 MSM of cfg.  tables: the call was a table call (one window whose entry
    w n + i is the table entry 2^(c w) P_i).  counts: a dict that receives the replayed classes of the accumulate
    kernel and the plan counters.  identity: also check the weighted identity of the window partials."""
    p = cfg.test_g2_last_plan()
    assert (p["c"], p["lone"], p["instances"], p["workspace"]) == (c, 1, 1, 0)
    W, nb, lb, n = p["W"], p["nb"], p["lb"], p["n"]
    assert p["n_scalars"] == len(ks) and nb == 1 << lb
    digits = st.np_signed_digits(ks, c, p["W_digits"])
    assert np.array_equal(_tap_digits(cfg, msm_pkg, p), digits), "digits"
    if tables:
        assert W == 1 and n == p["W_digits"] * len(ks)
        entry_dlogs = [a << (c * w) for w in range(p["W_digits"]) for a in dlogs]
        digits = digits.reshape(1, n)
    else:
        assert W == p["W_digits"] and n == len(ks)
        entry_dlogs = dlogs
    size = _u32(cfg, msm_pkg.STAGE_BUCKET_SIZE)
    exp_size = np.stack([np.bincount(np.abs(digits[w]), minlength=nb + 1)[1:] for w in range(W)])
    assert exp_size.shape == (W, nb), "a digit magnitude above 2^lb"
    assert np.array_equal(size, exp_size.reshape(-1)), "bucket sizes"
    sums, exp_b = sr.expected_buckets(digits, entry_dlogs, lb)
    nonempty = [int(i) for i in np.nonzero(size)[0]]
    assert nonempty == sorted(w * nb + s for w in range(W) for s in exp_b[w])
    got_b = sr.decode_records(cfg.test_g2_stage_copy(msm_pkg.STAGE_BUCKETS), which=nonempty)
    assert len(got_b) == W * nb
    bad = [i for i in nonempty if got_b[i] != exp_b[i >> lb][i & (nb - 1)]]
    assert not bad, f"{len(bad)} buckets differ; first: window {bad[0] >> lb} slot {bad[0] & (nb - 1)} size {size[bad[0]]}"
    _, exp_p = sr.expected_partials(sums, W, lb)
    got_p = sr.decode_records(cfg.test_g2_stage_copy(msm_pkg.STAGE_PARTIAL))
    assert len(got_p) == W * (lb + 1)
    bad = [i for i in range(len(got_p)) if got_p[i] != exp_p[i // (lb + 1)][i % (lb + 1)]]
    assert not bad, f"{len(bad)} window partials differ; first: window {bad[0] // (lb + 1)} term {bad[0] % (lb + 1)}"
    th.assert_result(out, th.expected(ks, dlogs))
    if identity:
        check_window_identity(got_p, sums, lb)
    if counts is not None:
        got = sr.replay_items(_u32(cfg, msm_pkg.STAGE_SORTED), _u32(cfg, msm_pkg.STAGE_BUCKET_START), size, n, W, lb,
                              p["CH"], entry_dlogs)
        for k, v in got.items():
            counts[k] = counts.get(k, 0) + v
        counts["multi_count"] = counts.get("multi_count", 0) + p["multi_count"]
        counts["deferred"] = counts.get("deferred", 0) + p["deferred"]
    return p


def run_g2(cfg, ks, pts, c, prepared=False):
    n = len(ks)
    cfg.set_window_size(c)
    d = None
    try:
        if not prepared:
            return cfg.msm_g2(le(ks), pts, n, scalar_layout=CANON)
        d = cfg.g2_bases_upload(pts, n)
        return cfg.msm_g2_prepared(le(ks), d, n, scalar_layout=CANON)
    finally:
        cfg.set_window_size(0)
        if d is not None:
            cfg.free(d)


# ---- accumulate and combine -----------------------------------------------------------------------------------------
CLASS_COUNTS = {}


@pytest.fixture(scope="module")
def constructed():
    ks, dl = sr.constructed_instance()
    return ks, dl, sr.encode_points(dl)


def run_constructed(cfg, msm_pkg, constructed, prepared, counts):
    ks, dl, pts = constructed
    out = run_g2(cfg, ks, pts, sr.CONSTRUCTED_C, prepared=prepared)
    p = cfg.test_g2_last_plan()
    assert p["CH"] == 16, "the constructed bucket sizes assume CH = 16"
    assert p["multi_count"] > 0 and p["deferred"] > 0
    check_g2_buckets(cfg, msm_pkg, ks, dl, out, sr.CONSTRUCTED_C, counts=counts)
    return out


@pytest.mark.parametrize("path", ["host_buffers", "prepared"])
def test_g2_accumulate_constructed_buckets(cfg, msm_pkg, constructed, path):
    out = run_constructed(cfg, msm_pkg, constructed, path == "prepared", CLASS_COUNTS)
    ks, dl, pts = constructed
    assert out == msm_pkg.host_msm_g2(le(ks), pts, len(ks), threads=4, scalar_layout=CANON)


def test_g2_branch_classes_all_reached(cfg, msm_pkg, constructed):
    """The coverage claim as a test: over this file's accumulate inputs every class of accumulate_g2_kernel's state
    machine occurred and both combine kernels ran.  (Runs the constructed input itself when the tests above were
    deselected.)"""
    counts = CLASS_COUNTS
    if not counts:
        run_constructed(cfg, msm_pkg, constructed, False, counts)
    print("\nG2 branch classes: " + ", ".join(f"{k}={v}" for k, v in counts.items()))
    missing = [k for k in sr.STEP_CLASSES + ("multi_count", "deferred") if counts.get(k, 0) == 0]
    assert not missing, f"branch classes never reached: {missing} ({counts})"


# ---- window partials: the shapes of reduce_bits_body and of the level planner -----------------------------------------
@pytest.mark.parametrize("c,n,threads", [(3, 40, 64), (8, 300, 64), (17, 200, 128)])
def test_g2_window_partials(cfg, msm_pkg, bases, c, n, threads):
    """c = 3: the padded window (rows and columns of 2 and 4 slots: 64 threads face one or two summands each);
    c = 8: several summands per thread, more than one level of group sums; c = 17: rows of 256 nearly empty slots,
    where the thread picker stops at the cap of 128."""
    dl, pts = bases
    rng = random.Random(c)
    edge = st._edge_scalars(c, rng)
    ks = [rng.randrange(g.R_ORDER) for _ in range(n - min(40, n // 2))] + edge[:min(40, n // 2)]
    out = run_g2(cfg, ks, pts[:128 * n], c)
    p = check_g2_buckets(cfg, msm_pkg, ks, dl[:n], out, c, counts=CLASS_COUNTS, identity=True)
    assert p["lb"] == max(c - 1, 3) and p["rb_threads"] == 0
    assert reduce_bits_threads(p["lb"]) == threads


# ---- the table pipeline -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", [(16, 512), (21, 64)])
def test_g2_tables_stages(cfg, msm_pkg, c, n):
    """One window of W_digits n entries; at c = 21 a row of 2^20 slots of which a few hundred hold anything.  Discrete
    logs below 2^24 keep 2^(c w) a_i at three or four non-zero bytes for the fixed-base table."""
    rng = random.Random(c)
    dl = sr.distinct_dlogs(rng, n, bits=24)
    dl[3] = 0                                      # an identity base stays the identity in every window's table
    pts = sr.encode_points(dl)
    ks = [rng.randrange(g.R_ORDER) for _ in range(n - 8)] + st._edge_scalars(c, rng)[:8]
    t = cfg.g2_tables_build(pts, n, window_size=c)
    try:
        info = cfg.g2_tables_info(t)
        assert info["window_size"] == c and info["num_windows"] * n < 1 << 31
        out = cfg.msm_g2_tables(le(ks), t, scalar_layout=CANON)
        p = check_g2_buckets(cfg, msm_pkg, ks, dl, out, c, counts=CLASS_COUNTS, tables=True)
        assert p["W"] == 1 and p["lb"] == c - 1
    finally:
        cfg.g2_tables_free(t)


# ---- stale workspaces -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_g2_poisoned_workspaces(cfg, msm_pkg, bases, byte):
    """run_msm_g2 does not clear its bucket matrix: the window reduction must take every empty slot as the identity
    from bucket_size alone.  Every point-valued buffer (the G2 ones included) is filled with a non-zero byte before
    every call of a sequence whose plans grow and shrink; every result must equal the model and the host G2 MSM."""
    dl, pts = bases
    rng = random.Random(byte)
    seq = [("c17", 17, [rng.randrange(g.R_ORDER) for _ in range(512)]),
           ("c3", 3, [rng.randrange(g.R_ORDER) for _ in range(40)]),
           ("c5_skewed", 5, [rng.choice([1, 2, 33, 1 << 200]) for _ in range(300)]),
           ("c15", 15, [rng.randrange(g.R_ORDER) for _ in range(512)]),
           ("zeros", 15, [0] * 512),
           ("c5", 5, [rng.randrange(g.R_ORDER) for _ in range(300)])]
    for name, c, ks in seq:
        n = len(ks)
        cfg.test_fill_workspaces(byte)
        out = run_g2(cfg, ks, pts[:128 * n], c)
        assert cfg.test_g2_last_plan()["c"] == c
        exp = th.expected(ks, dl[:n])
        assert (None if out == g.identity_bytes() else g.decode_jacobian(out)) == exp, f"{name}: differs after poisoning"
        th.assert_result(out, exp)
        assert out == msm_pkg.host_msm_g2(le(ks), pts[:128 * n], n, threads=4, scalar_layout=CANON), name
    t = cfg.g2_tables_build(pts, 512, window_size=16)
    try:
        ks = [rng.randrange(g.R_ORDER) for _ in range(512)]
        cfg.test_fill_workspaces(byte)
        out = cfg.msm_g2_tables(le(ks), t, scalar_layout=CANON)
        p = cfg.test_g2_last_plan()
        assert p["c"] == 16 and p["W"] == 1 and p["nb"] == 1 << 15
        th.assert_result(out, th.expected(ks, dl))
        assert out == msm_pkg.host_msm_g2(le(ks), pts, 512, threads=4, scalar_layout=CANON), "tables"
    finally:
        cfg.g2_tables_free(t)
    # a G1 call of the same ctx after the G2 calls, its workspaces poisoned as in test_poisoned_workspaces
    ks1 = [rng.randrange(g.R_ORDER) for _ in range(600)]
    pts1 = st._points(st.o.SEED_BASE + 400, 600)
    cfg.test_fill_workspaces(byte)
    out1 = st._run(cfg, msm_pkg, [(ks1, pts1)], c=8)[0]
    assert st._same_point(out1, st._expected(ks1, pts1)), "G1 after G2: result differs after poisoning"


# ---- the tap's own argument checks ------------------------------------------------------------------------------------
def _status(msm_pkg, fn, *args):
    with pytest.raises(msm_pkg.MsmError) as e:
        fn(*args)
    return e.value.status


def test_g2_tap_argument_errors(msm_pkg, bases):
    dl, pts = bases
    ctx = msm_pkg.MsmConfig(0)
    try:
        # before any G2 MSM
        assert _status(msm_pkg, ctx.test_g2_last_plan) == msm_pkg.INPUT_ERROR
        assert _status(msm_pkg, ctx.test_g2_stage_copy, msm_pkg.STAGE_BUCKET_SIZE) == msm_pkg.INPUT_ERROR
        rng = random.Random(77)
        n = 64
        ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
        out = ctx.msm_g2(le(ks), pts[:128 * n], n, scalar_layout=CANON)
        th.assert_result(out, th.expected(ks, dl[:n]))
        plan = ctx.test_g2_last_plan()
        taps = {w: ctx.test_g2_stage_copy(w) for w in range(10)}
        assert len(taps[msm_pkg.STAGE_BUCKETS]) == 192 * plan["W"] * plan["nb"]
        assert len(taps[msm_pkg.STAGE_PARTIAL]) == 192 * plan["W"] * (plan["lb"] + 1)
        # a wrong *bytes and an unknown buffer id
        L = msm_pkg.lib()
        want = ctypes.c_size_t(0)
        assert L.msm_amd_test_g2_stage_copy(ctx.h, msm_pkg.STAGE_PARTIAL, None, ctypes.byref(want)) == 0
        buf = ctypes.create_string_buffer(want.value + 192)
        for wrong in (want.value - 192, want.value + 192, 0):
            nbytes = ctypes.c_size_t(wrong)
            assert L.msm_amd_test_g2_stage_copy(ctx.h, msm_pkg.STAGE_PARTIAL, buf, ctypes.byref(nbytes)) == msm_pkg.INPUT_ERROR
        assert buf.raw == bytes(want.value + 192), "a refused copy wrote into the buffer"
        for which in (10, 99, -1):
            assert _status(msm_pkg, ctx.test_g2_stage_copy, which) == msm_pkg.INPUT_ERROR
        assert L.msm_amd_test_g2_stage_copy(ctx.h, msm_pkg.STAGE_PARTIAL, buf, None) == msm_pkg.INPUT_ERROR
        # a G1 call in between changes nothing of what the G2 tap reports
        ks1 = [rng.randrange(g.R_ORDER) for _ in range(300)]
        pts1 = st._points(st.o.SEED_BASE + 401, 300)
        out1 = st._run(ctx, msm_pkg, [(ks1, pts1)], c=8)[0]
        assert st._same_point(out1, st._expected(ks1, pts1))
        assert ctx.test_last_plan()["c"] == 8
        assert ctx.test_g2_last_plan() == plan
        assert {w: ctx.test_g2_stage_copy(w) for w in range(10)} == taps
        # after a failed G2 MSM (no such table handle: refused before anything is enqueued) the tap reads nothing
        ds = ctx.alloc(32 * n)
        try:
            assert _status(msm_pkg, ctx.msm_g2_device, ds, 0x1234, n, CANON, msm_pkg.G2_POINT_TABLES) == msm_pkg.INPUT_ERROR
        finally:
            ctx.free(ds)
        assert _status(msm_pkg, ctx.test_g2_last_plan) == msm_pkg.INPUT_ERROR
        assert _status(msm_pkg, ctx.test_g2_stage_copy, msm_pkg.STAGE_PARTIAL) == msm_pkg.INPUT_ERROR
    finally:
        ctx.close()
