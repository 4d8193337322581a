"""The fused sort front end, through the stage tap: digits_hist_kernel (digits and the pass-1 region counts in one
kernel) and the packed pass-1 payload (fine | index << fb | sign << 31 in one u32, no tmp_fine).

Every case checks, against numpy signed digits of the scalars it sent:
  digit matrix   exact
  bucket_size    exact
  sorted         per window and slot exactly the multiset of (index, sign) with that digit
(check_sort_plan of test_gpu_pipeline_stages.py, which also checks the scans and the item order), and asserts which
path the plan took (plan words fused_front / packed)."""
import random

import numpy as np
import pytest

import g2_ref as g
import test_gpu_pipeline_stages as st
from oracle import bn254_ref as o

pytestmark = pytest.mark.gpu


def _check(cfg, msm_pkg, ks, c, plan, j=0, fused=1, packed=1, windows=None):
    assert (plan["fused_front"], plan["packed"]) == (fused, packed), plan
    exp = st.np_signed_digits(ks, c, plan["W_digits"])
    got = st._tap_digits(cfg, msm_pkg, plan, j)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"first wrong digit (window, scalar) {tuple(bad[0])}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"
    st.check_sort_plan(cfg, msm_pkg, exp, j=j, windows=windows)


def _scalars(c, n, seed, canonical):
    """Random scalars with the edge scalars of the window size, zeros, scalars whose high windows are all zero, and (in
    the canonical layout) values in [r, 2^256)."""
    rng = random.Random(seed)
    ks = st._edge_scalars(c, rng)[:n // 4]
    ks += [0] * (n // 16) + [rng.randrange(1 << (2 * c)) for _ in range(n // 16)]
    if canonical:
        ks += [o.R_ORDER, o.R_ORDER + 1, (1 << 256) - 1, 5 * o.R_ORDER + 3][:max(0, n - len(ks))]
    ks += [rng.randrange(o.R_ORDER) for _ in range(n - len(ks))]
    rng.shuffle(ks)
    assert len(ks) == n
    return ks


# n = 9001: three chunks of 3008 scalars, the last one short; n = 1000: less than one chunk
@pytest.mark.parametrize("layout", ["mont", "canonical"])
@pytest.mark.parametrize("n", [9001, 1000])
@pytest.mark.parametrize("c", [8, 13, 15, 16, 17])
def test_fused_front_lone(cfg, msm_pkg, c, n, layout):
    """The four specialisations of digits_hist_kernel and the generic form (c = 8), both scalar layouts, a lone call."""
    canonical = layout == "canonical"
    ks = _scalars(c, n, c * 1000 + n + canonical, canonical)
    pts = st._points(o.SEED_BASE + c + n, n)
    out = st._run(cfg, msm_pkg, [(ks, pts)], c=c, canonical=canonical)[0]
    plan = cfg.test_last_plan()
    assert plan["lone"] == 1 and plan["c"] == c and plan["mb"] == 0
    if n == 9001:
        assert plan["Q"] > 1 and n % plan["Q"] != 0
    else:
        assert plan["Q"] == 1
    _check(cfg, msm_pkg, ks, c, plan)
    assert st._same_point(out, st._expected([k % o.R_ORDER for k in ks], pts))


def test_fused_front_pipelined(cfg, msm_pkg):
    """Three instances in one batch (front ends on their own stream beside the accumulate grids), sizes that differ."""
    c = 15
    insts = []
    for i in range(3):
        n = 20000 + 4097 * i
        insts.append((_scalars(c, n, 77 + i, False), st._points(o.SEED_BASE + 900 + i, n)))
    outs = st._run(cfg, msm_pkg, insts, c=c)
    for j, (ks, pts) in enumerate(insts):
        plan = cfg.test_last_plan(j)
        assert plan["lone"] == 0 and plan["hb"] > 0
        _check(cfg, msm_pkg, ks, c, plan, j=j)
        assert st._same_point(outs[j], st._expected(ks, pts))


@pytest.mark.parametrize("c", [15, 17])
def test_all_digits_equal_fine_fallback(cfg, msm_pkg, c):
    """40 000 equal scalars: one coarse region of every window takes everything, larger than the LDS staging of pass 2
    (kFineCap = 28 672), so the packed payload goes through fine_sort_kernel's global fallback."""
    n = 40000
    ks = [0x1234_5678_9ABC_DEF0_1357_9BDF_0246_8ACE_1122_3344_5566_7788] * n
    pts = st._points(o.SEED_BASE + 40000 + c, n)
    out = st._run(cfg, msm_pkg, [(ks, pts)], c=c)[0]
    plan = cfg.test_last_plan()
    assert plan["hb"] > 0
    _check(cfg, msm_pkg, ks, c, plan)
    assert st._same_point(out, st._expected(ks, pts))


def test_all_zero_scalars(cfg, msm_pkg):
    """No entry at all: every counter, region and bucket is empty."""
    n = 5000
    ks = [0] * n
    pts = st._points(o.SEED_BASE + 5000, n)
    st._run(cfg, msm_pkg, [(ks, pts)], c=15)
    plan = cfg.test_last_plan()
    _check(cfg, msm_pkg, ks, 15, plan)
    assert plan["total_items"] == 0


def test_unpacked_path_2p22(cfg, msm_pkg):
    """A lone 2^22-point call sorts in three levels: the payload stays two arrays (packed = 0) behind the fused
    histogram.  Digits are checked for 4096 scalars (chunk borders included), the sort against the tapped matrix."""
    n = 1 << 22
    dp, ds = cfg.generate_instance(o.SEED_BASE + 2222, n, False)   # canonical scalars
    try:
        raw = cfg.to_host(ds, 32 * n)
        cfg.msm_batch_device([ds], [dp], [n], msm_pkg.SCALAR_CANON_LE)
    finally:
        cfg.free(dp)
        cfg.free(ds)
    plan = cfg.test_last_plan()
    assert plan["lone"] == 1 and plan["mb"] > 0
    assert (plan["fused_front"], plan["packed"]) == (1, 0), plan
    c, W = plan["c"], plan["W_digits"]
    chunk = (((n + plan["Q"] - 1) // plan["Q"]) + 63) & ~63
    rng = random.Random(22)
    idx = sorted({i for i in (0, n - 1, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, (plan["Q"] - 1) * chunk) if i < n} |
                 {rng.randrange(n) for _ in range(4096)})
    ks = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in idx]
    digits = st._tap_digits(cfg, msm_pkg, plan)
    assert np.array_equal(digits[:, idx], st.np_signed_digits(ks, c, W))
    st.check_sort_plan(cfg, msm_pkg, digits, windows=[0, plan["W"] // 2, plan["W"] - 1])


def test_tables_keep_two_kernel_front(cfg, msm_pkg):
    """The table pipeline consumes the digit matrix as ONE window with another chunking: digits_kernel and
    coarse_hist_kernel stay; its entries may still be packed."""
    n = 2048
    rng = random.Random(5)
    ks = [rng.randrange(o.R_ORDER) for _ in range(n)]
    pts = st._points(o.SEED_BASE + 2048, n)
    tables = cfg.tables_build(pts, n, window_size=16)
    try:
        out = cfg.msm_tables(st._mont_bytes(ks), tables)
        plan = cfg.test_last_plan()
        assert plan["W"] == 1 and plan["fused_front"] == 0, plan
        digits = st._tap_digits(cfg, msm_pkg, plan)
        assert np.array_equal(digits, st.np_signed_digits(ks, 16, plan["W_digits"]))
        st.check_sort_plan(cfg, msm_pkg, digits)
        assert st._same_point(out, st._expected(ks, pts))
    finally:
        cfg.tables_free(tables)


def test_g2_call_takes_fused_front(cfg, msm_pkg):
    """run_msm_g2 shares the front end: one G2 MSM (c = 15, 2^14 points) against the host G2 MSM."""
    n = 1 << 14
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(31337, g.GEN2)), g.encode_h2c(g.scalar_mul(271828, g.GEN2)), n)
    words = np.random.default_rng(14).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    words[:, 7] &= 0x0FFFFFFF   # < 2^252 < r
    words[::7] = 0              # zero scalars
    sc = words.tobytes()
    assert cfg.msm_g2(sc, pts, n, scalar_layout=msm_pkg.SCALAR_CANON_LE) == \
        msm_pkg.host_msm_g2(sc, pts, n, threads=8, scalar_layout=msm_pkg.SCALAR_CANON_LE)
