"""CPU-only tests of the persistent G2 bases / G2 window tables: the new symbols and layout rules, the inversion and
the XYZZ -> affine step of the 29-bit G2 arithmetic (through their host twins) against big integers at the edges of
their bounds contract, and the host twin of the table build against scalar multiplications of the model."""
import random

import pytest

import g2_ref as g
import test_g2_host as th

NEW_SYMBOLS = ["msm_amd_g2_bases_upload", "msm_amd_g2_bases_prepare_device", "msm_amd_msm_g2_prepared",
               "msm_amd_g2_tables_build", "msm_amd_g2_tables_build_device", "msm_amd_g2_tables_info",
               "msm_amd_g2_tables_free", "msm_amd_msm_g2_tables", "msm_amd_test_g2_tables_read",
               "msm_amd_test_g2_table_host"]
NEW_METHODS = ["g2_bases_upload", "g2_bases_prepare_device", "msm_g2_prepared", "g2_tables_build",
               "g2_tables_build_device", "g2_tables_info", "g2_tables_free", "msm_g2_tables", "g2_tables_read"]
RP = g.P / g.RHO


# ---- 1. symbols, layouts, refusals ------------------------------------------------------------------------------------
def test_new_symbols_and_layout_rules(msm_pkg):
    L = msm_pkg.lib()
    for s in NEW_SYMBOLS:
        assert s in msm_pkg.EXPORTS and hasattr(L, s), s
    for m in NEW_METHODS:
        assert callable(getattr(msm_pkg.MsmConfig, m)), m
    assert callable(msm_pkg.g2_table_host)
    assert (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, msm_pkg.G2_PREPARED_BYTES) == (2, 3, 128)
    assert (msm_pkg.G2_RAW_FQ2_INV, msm_pkg.G2_RAW_PT_TO_AFFINE) == (7, 8)
    # msm_amd_g2_point_bytes stays "bytes of a HOST layout"
    assert msm_pkg.g2_point_bytes(2) == 0 and msm_pkg.g2_point_bytes(3) == 0
    assert msm_pkg.g2_point_bytes(0) == 128 and msm_pkg.g2_point_bytes(1) == 136


@pytest.mark.parametrize("layout", [2, 3])
def test_host_entry_points_refuse_device_only_layouts(msm_pkg, layout):
    with pytest.raises(msm_pkg.MsmError) as e:
        msm_pkg.host_msm_g2(bytes(32), bytes(128), 1, point_layout=layout)
    assert e.value.status == msm_pkg.INPUT_ERROR
    L = msm_pkg.lib()
    out = bytes(192)
    # the argument checks come before anything touches the pointers: an address nobody could read, and no ctx
    assert L.msm_amd_host_msm_g2(0, layout, 8, 8, 4, 1, out) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_msm_g2(None, 0, layout, 8, 8, 4, out) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_test_g2_table_host(layout, 8, 4, 4, 64, 1, out) == msm_pkg.INPUT_ERROR


def test_raw_op_numbering_is_bounded(msm_pkg):
    L = msm_pkg.lib()
    a = (msm_pkg.c_uint32 * 72)()
    out = (msm_pkg.c_uint32 * 80)()
    assert L.msm_amd_test_op_g2_host(9, a, a, out, 1) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_test_op_g2_host(-1, a, a, out, 1) == msm_pkg.INPUT_ERROR


# ---- 2. inversion and to-affine on raw limbs --------------------------------------------------------------------------
def inv_corpus(seed, n=60):
    """operands of Fq2::inv at the edges of its contract: a != 0, each component a random multiple of p below 32 p (the
    top one half the time), limbs normalised with borrowed limbs; one component zero in some"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        a = g.rand_fq2(rng)
        if i % 10 == 0:
            a = (0, a[1])
        if i % 10 == 5:
            a = (a[0], 0)
        if i == 1:
            a = (1, 0)
        if i == 2:
            a = (g.P - 1, g.P - 1)
        ma = (rng.choice([1, 2, 20, 32]), rng.choice([1, 2, 20, 32]))
        out.append(g.fq2_rec(a, ma, rng))
    return out


def check_inv(aw, ow):
    """a out = 1 in big integers; out meets the header's bound: multiplication outputs (exact limbs) below
    (1 + rho' 32 * 1.08) p < 1.21 p"""
    a, r = g.fq2_of(aw), g.fq2_of(ow)
    assert g.mul2(a, r) == g.ONE2
    assert all(v < 32 for v in g.component_multiples(aw, 2))
    m = g.component_multiples(ow, 2)
    assert max(m) < 1 + RP * 32 * 1.08 < 1.21, m
    assert all(ow[k] < (1 << 29) for k in list(range(8)) + list(range(9, 17)))
    assert ow[18:72] == [0] * 54 and ow[72] == 0


def test_raw_fq2_inv_host(msm_pkg):
    cases = inv_corpus(21)
    a = [w for x in cases for w in g.pad(x)]
    out = msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_FQ2_INV, a, [0] * len(a), len(cases))
    for i, x in enumerate(cases):
        check_inv(x, out[80 * i:80 * i + 80])


def affine_corpus(seed, n=24):
    """XYZZ records inside the point invariant (random Z, coordinates at random multiples of p up to the bounds) and
    records with ZZ = ZZZ = 1 (an affine entry restarted), with the affine point they stand for"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        p = th._point(rng.randrange(1, 1 << 60))
        z = g.ONE2 if i % 6 == 0 else None
        w = g.xyzz_rec(p, rng, z=z)
        out.append((w, p))
    return out


def check_affine(aw, ow, pt):
    assert g.decode_xyzz(aw) == pt
    x, y = g.fq2_of(ow[0:18]), g.fq2_of(ow[18:36])
    assert (x, y) == pt
    assert all(g.value(ow[9 * i:9 * i + 9]) < g.P for i in range(4))          # canonical values ...
    assert all(ow[9 * i + k] < (1 << 29) for i in range(4) for k in range(9))  # ... in exact limbs
    assert ow[36:80] == [0] * 44


def test_raw_pt_to_affine_host(msm_pkg):
    cases = affine_corpus(22)
    a = [w for c in cases for w in c[0]]
    out = msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_PT_TO_AFFINE, a, [0] * len(a), len(cases))
    for i, (w, pt) in enumerate(cases):
        check_affine(w, out[80 * i:80 * i + 80], pt)


def test_bounds_model_covers_the_inversion():
    import os
    import subprocess
    r = subprocess.run(["python3", os.path.join(th.ROOT, "tools", "g2_bounds.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "invariant" in r.stdout and "affine.x" in r.stdout and "inv(32p)" in r.stdout


# ---- 3. the host twin of the table build against big integers ---------------------------------------------------------
def table_points(seed, n=30):
    rng = random.Random(seed)
    pts = [g.rand_point(rng) for _ in range(n)]
    pts[3] = None
    pts[n - 1] = None
    pts[7] = pts[6]
    pts[9] = g.neg(pts[8])
    pts[0] = g.GEN2
    return pts


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("c", [4, 7, 16, 21])
def test_g2_table_host_against_scalar_mul(msm_pkg, c, layout):
    n = 30
    W = 254 // c + 1
    pts = table_points(300 + c, n)
    enc = g.encode_h2c if layout == 0 else g.encode_ark
    tab = msm_pkg.g2_table_host(b"".join(enc(p) for p in pts), n, c, W, threads=4, point_layout=layout)
    assert len(tab) == 128 * n * W
    entries = [(w, i) for w in range(W) for i in range(n)]
    if len(entries) > 500:   # large table: a fixed sample, all of the top window and of window 0 included
        rng = random.Random(c)
        entries = ([(W - 1, i) for i in range(n)] + [(0, i) for i in range(n)] + [(1, i) for i in range(0, n, 3)] +
                   [(rng.randrange(2, W - 1), rng.randrange(n)) for _ in range(40)])
        assert len(entries) >= 64
    for w, i in entries:
        rec = tab[128 * (w * n + i):128 * (w * n + i) + 128]
        if pts[i] is None:
            assert rec == bytes(128), (w, i)
            continue
        assert g.decode_h2c(rec) == g.scalar_mul(1 << (c * w), pts[i]), (w, i)
        assert g.encode_h2c(g.decode_h2c(rec)) == rec, (w, i)   # canonical Montgomery words


def test_g2_table_host_is_thread_independent(msm_pkg):
    pts = table_points(5, 12)
    buf = b"".join(g.encode_h2c(p) for p in pts)
    assert msm_pkg.g2_table_host(buf, 12, 9, 29, threads=1) == msm_pkg.g2_table_host(buf, 12, 9, 29, threads=5)
