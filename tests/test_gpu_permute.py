"""halo2's permuted lookup columns on the GPU (msm_amd_fr_lookup_permute) against the host twin and the big-integer model of
tests/permute_ref.py (tests/test_permute_host.py pins the twin to the model on the CPU).  Every comparison is of bytes:
ctx call = twin = model, from a handle built from host rows and one built from device rows, into buffers that start as 0xFF
bytes, and every output passes check_halo2.  MSM_AMD_PERMUTE_TILE_LOG shortens the tiles of the integer scan so that a few
hundred rows take three to five levels; MSM_AMD_LOOKUP_HASH_BITS and MSM_AMD_LOOKUP_COUNT reach the probe,
MSM_AMD_PERMUTE_FILL the fill.  No byte depends on any of them.  The library has no form on device-resident buffers yet, so
the guard bands lie round the host buffers the call copies back into (tests/guard.py, HostArena)."""
import ctypes
import random

import pytest

import lookup_ref as lr
import permute_ref as pr
from guard import HostArena

pytestmark = pytest.mark.gpu

R = pr.R
FF = b"\xFF"


def handles_of(cfg, table, layout):
    """a handle built from host rows and one built from device rows, which are overwritten afterwards"""
    d_table = cfg.alloc(max(32, len(table)))
    try:
        cfg.to_device(d_table, table)
        hs = [cfg.fr_lookup_build(table, layout), cfg.fr_lookup_build_device(d_table, len(table) // 32, layout)]
        cfg.to_device(d_table, b"\xEE" * len(table))
    finally:
        cfg.free(d_table)
    return hs


def prefilled(nbytes):
    return ctypes.create_string_buffer(FF * nbytes, nbytes)


def check(cfg, msm_pkg, table, data, layout, n_vec=1, tag=None):
    """ctx call = twin = model, both outputs together and each alone; the outputs start as 0xFF bytes; the inputs are left
    as they were.  Returns (A', S', report)."""
    exp_a, exp_s, exp_rep = pr.permute(table, data, layout, n_vec)
    assert msm_pkg.host_fr_lookup_permute(table, data, layout, n_vec) == (exp_a, exp_s, exp_rep), tag
    pr.check_halo2(data, table, exp_a, exp_s, layout, n_vec)
    hs = handles_of(cfg, table, layout)
    try:
        for h in hs:
            src, a, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data)), prefilled(len(data))
            assert cfg.fr_lookup_permute(h, src, layout, n_vec, a_out=a, s_out=s) == (None, None, exp_rep), tag
            assert pr.first_difference(a.raw, exp_a) is None, tag
            assert pr.first_difference(s.raw, exp_s) is None, tag
            assert src.raw == data, tag
            assert cfg.fr_lookup_permute(h, data, layout, n_vec, want_s=False) == (exp_a, None, exp_rep), tag
            assert cfg.fr_lookup_permute(h, data, layout, n_vec, want_a=False) == (None, exp_s, exp_rep), tag
    finally:
        for h in hs:
            h.free()
    return exp_a, exp_s, exp_rep


# ---- 1. sizes across the wave and the workgroup ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(cfg, msm_pkg, n):
    for layout in pr.LAYOUTS:
        table = lr.random_table(n + layout, n, layout, distinct=max(1, n - n // 4))
        check(cfg, msm_pkg, table, pr.column("uniform", n, table, layout, n), layout, tag=(n, layout))


# ---- 2. plans of three, four and five levels that end in partial tiles -----------------------------------------------------------
@pytest.mark.parametrize("n,levels", [(17, 3), (65, 4), (300, 5)])
def test_many_level_plans(cfg, msm_pkg, n, levels, monkeypatch):
    layout = pr.CANON_LE
    table = lr.random_table(n, n, layout, distinct=n - n // 3)
    cols = b"".join(pr.column(kind, n + k, table, layout, n) for k, kind in enumerate(("uniform", "half")))
    default = check(cfg, msm_pkg, table, cols, layout, 2, tag=(n, "default"))
    monkeypatch.setenv("MSM_AMD_PERMUTE_TILE_LOG", "2")
    assert msm_pkg.test_fr_permute_plan(n, 2, 2)["levels"] == levels
    assert check(cfg, msm_pkg, table, cols, layout, 2, tag=(n, "tiles of 4")) == default


# ---- 3. skew: one row takes every input, or half of them ----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_skew(cfg, msm_pkg, layout):
    n = 700
    table = lr.random_table(31, n, layout)
    rows = pr.decode(table, layout)
    for j in (0, n - 1, 350):
        a, s, rep = check(cfg, msm_pkg, table, pr.column("row%d" % j, 1, table, layout, n), layout, tag=j)
        assert pr.decode(a, layout) == [rows[j]] * n
        assert pr.decode(s, layout) == [rows[j]] + rows[:j] + rows[j + 1:]     # that row, then all others ascending
        assert rep == dict(n_missing=0, first_missing=pr.NO_MISS, rows_hit=1, max_multiplicity=n)
    a, s, rep = check(cfg, msm_pkg, table, pr.column("half", 2, table, layout, n), layout, tag="half")
    assert rep["max_multiplicity"] >= n // 2


# ---- 4. no repeats: every position is a head -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_no_repeats(cfg, msm_pkg, layout):
    table = lr.random_table(41, 513, layout)
    a, s, rep = check(cfg, msm_pkg, table, pr.column("shuffle", 3, table, layout, 513), layout)
    assert a == s == table and rep["rows_hit"] == 513 and rep["max_multiplicity"] == 1


# ---- 5. rows that are equal mod r under different words -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_rows_equal_mod_r(cfg, msm_pkg, layout):
    table = lr.edge_records(layout) + pr.encode([5, 7], layout)
    vals = pr.decode(table, layout)
    data = pr.raw([R, 0, R + 5, 5]) + pr.encode([vals[1], vals[1], vals[7], vals[5]], layout)
    a, s, rep = check(cfg, msm_pkg, table, data, layout, tag="edge")
    assert pr.decode(a, layout)[:2] == [vals[0], vals[0]] and pr.decode(s, layout)[1] == vals[2]
    check(cfg, msm_pkg, pr.raw([R + 5, 5, R, 0]), pr.raw([5, 0, R + 5, 2 * R]), layout, tag="r + 5 beside 5")


# ---- 6. several columns: a column boundary inside a tile and inside a wave ----------------------------------------------------------
@pytest.mark.parametrize("count", ["block", "wave", "lane"])
@pytest.mark.parametrize("n", [65, 257])
def test_several_columns(cfg, msm_pkg, n, count, monkeypatch):
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    layout = pr.MONT_LE
    table = lr.random_table(n, n, layout, distinct=n - 9)
    cols = [pr.column(kind, k, table, layout, n) for k, kind in enumerate(("uniform", "row%d" % (n - 1), "shuffle"))]
    a, s, rep = check(cfg, msm_pkg, table, b"".join(cols), layout, 3, tag=(n, count))
    for k, col in enumerate(cols):                                # no counter of a column leaks into the next
        one = pr.permute(table, col, layout)
        assert (a[32 * n * k:32 * n * (k + 1)], s[32 * n * k:32 * n * (k + 1)]) == one[:2], (n, k)


# ---- 7. output combinations -----------------------------------------------------------------------------------------------------------
def test_output_combinations(cfg, msm_pkg):
    layout = pr.MONT_LE
    table = lr.random_table(3, 100, layout, distinct=60)
    hs = handles_of(cfg, table, layout)
    try:
        for h in hs:
            for n in (7, 333):                                    # a_out alone: n < n_rows and n > n_rows
                data = pr.column("uniform", n, table, layout, n)
                exp_a, _, exp_rep = pr.permute(table, data, layout, want_s=False)
                assert msm_pkg.host_fr_lookup_permute(table, data, layout, want_s=False) == (exp_a, None, exp_rep)
                assert cfg.fr_lookup_permute(h, data, layout, want_s=False) == (exp_a, None, exp_rep)
                a, s = prefilled(len(data)), prefilled(len(data))
                with pytest.raises(msm_pkg.MsmError) as e:        # s_out with n != n_rows
                    cfg.fr_lookup_permute(h, data, layout, a_out=a, s_out=s)
                assert e.value.status == msm_pkg.INPUT_ERROR and "n == n_rows" in str(e.value)
                assert a.raw == s.raw == FF * len(data)
                buf = ctypes.create_string_buffer(data, len(data))                                       # in place
                assert cfg.fr_lookup_permute(h, buf, layout, want_s=False, a_out=buf) == (None, None, exp_rep)
                assert buf.raw == exp_a
            data = pr.column("half", 5, table, layout, 100)
            exp_a, exp_s, exp_rep = pr.permute(table, data, layout)
            s = prefilled(len(data))
            assert cfg.fr_lookup_permute(h, data, layout, want_a=False, s_out=s) == (None, None, exp_rep)   # s_out alone
            assert s.raw == exp_s
            buf, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data))                  # in place, with S'
            assert cfg.fr_lookup_permute(h, buf, layout, a_out=buf, s_out=s) == (None, None, exp_rep)
            assert (buf.raw, s.raw) == (exp_a, exp_s)
            zero = dict.fromkeys(msm_pkg.LOOKUP_REPORT_FIELDS, 0)
            rep = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
            s = prefilled(len(data))
            L = msm_pkg.lib()
            assert L.msm_amd_fr_lookup_permute(cfg.h, h.h, layout, buf, 0, 1, buf, s, rep) == msm_pkg.OK    # n = 0
            assert list(rep) == [0, 0, 0, 0]
            rep[:] = [9, 9, 9, 9]
            assert L.msm_amd_fr_lookup_permute(cfg.h, h.h, layout, buf, 100, 0, buf, s, rep) == msm_pkg.OK  # n_vec = 0
            assert list(rep) == [0, 0, 0, 0] and s.raw == FF * len(data) and buf.raw == exp_a
            assert cfg.fr_lookup_permute(h, b"", layout) == (b"", b"", zero)
    finally:
        for h in hs:
            h.free()


def test_argument_errors(cfg, msm_pkg):
    L = msm_pkg.lib()
    layout = pr.MONT_LE
    table = lr.random_table(3, 64, layout)
    data = pr.column("uniform", 1, table, layout, 64)
    h = cfg.fr_lookup_build(table, layout)
    other = msm_pkg.setup_metal_state()
    try:
        big = ctypes.create_string_buffer(data * 4, 4 * len(data))
        at = ctypes.addressof(big)
        rep = (ctypes.c_uint64 * 4)()
        P = ctypes.c_void_p
        good = dict(h=h.h, layout=layout, src=at, n=64, n_vec=1, a=at + 2048, s=at + 4096, rep=rep)

        def call(**kw):
            x = dict(good, **kw)
            return L.msm_amd_fr_lookup_permute(cfg.h, x["h"], x["layout"], P(x["src"]), x["n"], x["n_vec"], P(x["a"]), P(x["s"]),
                                               x["rep"])
        assert call() == msm_pkg.OK
        before, image = big.raw, h.info()["device_bytes"]
        errors = dict(unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), null_in=dict(src=None), null_report=dict(rep=None),
                      no_output=dict(a=None, s=None), s_with_other_n=dict(n=63), foreign_handle=dict(h=P(at)),
                      a_over_in=dict(a=at + 32), s_is_in=dict(s=at), s_over_a=dict(s=at + 2048 + 32 * 63),
                      n_2_32=dict(n=1 << 32, s=None), product_2_32=dict(n=1 << 16, n_vec=1 << 16, s=None),
                      rows_product_2_32=dict(n=64, n_vec=1 << 26))
        for name, kw in errors.items():
            assert call(**kw) == msm_pkg.INPUT_ERROR, name
            assert b"msm_amd_fr_lookup_permute" in L.msm_amd_last_error(cfg.h), name
        assert big.raw == before and image == h.info()["device_bytes"]
        assert L.msm_amd_fr_lookup_permute(other.h, h.h, layout, data, 64, 1, P(at + 2048), None,
                                           rep) == msm_pkg.INPUT_ERROR               # a handle of another ctx
        h2 = cfg.fr_lookup_build(table, layout)
        h2.free()
        assert call(h=h2.h) == msm_pkg.INPUT_ERROR                 # a freed handle
        assert big.raw == before
    finally:
        other.close()
        h.free()


# ---- 8. misses --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss_at", [(4,), (100,), (194,), (0, 64, 129, 194)])
def test_misses(cfg, msm_pkg, miss_at):
    layout, n, n_vec = pr.CANON_LE, 65, 3
    table = lr.random_table(3, n, layout, distinct=40)
    data = lr.draws(11, table, layout, n * n_vec, miss_at)
    _, _, exp_rep = pr.permute(table, data, layout, n_vec)
    assert exp_rep["n_missing"] == len(miss_at) and exp_rep["first_missing"] == miss_at[0]
    hs = handles_of(cfg, table, layout)
    try:
        for h in hs:
            src, a, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data)), prefilled(len(data))
            with pytest.raises(msm_pkg.MsmError) as e:
                cfg.fr_lookup_permute(h, src, layout, n_vec, a_out=a, s_out=s)
            assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep, (e.value.report, exp_rep)
            assert "first at flat index %d " % miss_at[0] in str(e.value) and "%d of %d" % (len(miss_at), n * n_vec) in str(e.value)
            assert a.raw == s.raw == FF * len(data) and src.raw == data
            with pytest.raises(msm_pkg.MsmError):                 # in place: the inputs stay
                cfg.fr_lookup_permute(h, src, layout, n_vec, a_out=src, s_out=s)
            assert src.raw == data and s.raw == FF * len(data)
    finally:
        for h in hs:
            h.free()


# ---- 9. the knobs of the probe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ["block", "wave", "lane"])
@pytest.mark.parametrize("bits", ["0", "3"])
def test_probe_knobs_give_the_same_bytes(cfg, msm_pkg, bits, count, monkeypatch):
    layout = pr.MONT_LE
    table = lr.random_table(43, 257, layout, distinct=200)
    cols = b"".join(pr.column(kind, k, table, layout, 257) for k, kind in enumerate(("half", "uniform")))
    default = pr.permute(table, cols, layout, 2)
    monkeypatch.setenv("MSM_AMD_LOOKUP_HASH_BITS", bits)
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    assert check(cfg, msm_pkg, table, cols, layout, 2, tag=(bits, count)) == default


@pytest.mark.parametrize("tile_log", ["11", "2"])
def test_fill_forms_give_the_same_bytes(cfg, msm_pkg, tile_log, monkeypatch):
    """MSM_AMD_PERMUTE_FILL=scan: the owner of a position from a maximum scan over the scattered heads, not from the search;
    three columns of 300 positions, at tiles of 4 a five-level scan whose column boundaries fall inside tiles"""
    layout = pr.CANON_LE
    table = lr.random_table(47, 300, layout, distinct=211)
    cols = b"".join(pr.column(kind, k, table, layout, 300) for k, kind in enumerate(("half", "row299", "shuffle")))
    monkeypatch.setenv("MSM_AMD_PERMUTE_TILE_LOG", tile_log)
    monkeypatch.setenv("MSM_AMD_PERMUTE_FILL", "scan")
    check(cfg, msm_pkg, table, cols, layout, 3, tag=("scan", tile_log))
    h = cfg.fr_lookup_build(table, layout)
    try:
        for n in (1, 77, 1000):                                   # A' alone, n != n_rows: the owner words are n per column
            data = pr.column("uniform", n, table, layout, 2 * n)
            exp_a, _, exp_rep = pr.permute(table, data, layout, 2, want_s=False)
            assert cfg.fr_lookup_permute(h, data, layout, 2, want_s=False) == (exp_a, None, exp_rep), n
        data = lr.draws(3, table, layout, 300, (150,))
        a, s = (ctypes.create_string_buffer(FF * len(data), len(data)) for _ in range(2))
        with pytest.raises(msm_pkg.MsmError):
            cfg.fr_lookup_permute(h, data, layout, a_out=a, s_out=s)
        assert a.raw == s.raw == FF * len(data)
    finally:
        h.free()


# ---- 10. guard bands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_guard_bands(cfg, msm_pkg, n):
    """The host buffers the call copies back into: nothing outside a_out and s_out, nothing at all on a miss.  This holds the
    sizes of the copies back and the in-place rule.  It cannot see a kernel store outside the staged outputs (those lie in
    memory the ctx owns), nor whether the fill kernel itself obeys the miss counter (the call skips the copy back on the
    host): both need a call on the caller's device buffers, which the library does not have yet."""
    L = msm_pkg.lib()
    P = ctypes.c_void_p
    layout = pr.MONT_LE
    table = lr.random_table(n, n, layout, distinct=n - 20)
    data = pr.column("half", n, table, layout, n)
    exp_a, exp_s, exp_rep = pr.permute(table, data, layout)
    h = cfg.fr_lookup_build(table, layout)
    rep = (ctypes.c_uint64 * 4)()
    try:
        with HostArena() as arena:
            arena.add("in", data=data, readonly=True)
            arena.add("a", 32 * n)
            arena.add("s", 32 * n)
            arena.commit()
            assert L.msm_amd_fr_lookup_permute(cfg.h, h.h, layout, P(arena.ptr("in")), n, 1, P(arena.ptr("a")), P(arena.ptr("s")),
                                               rep) == msm_pkg.OK
            arena.verify()
            assert dict(zip(msm_pkg.LOOKUP_REPORT_FIELDS, rep)) == exp_rep and arena.get("a") == exp_a and arena.get("s") == exp_s
            arena.set("in", lr.draws(5, table, layout, n, (n - 1,)))
            arena.commit()
            assert L.msm_amd_fr_lookup_permute(cfg.h, h.h, layout, P(arena.ptr("in")), n, 1, P(arena.ptr("a")), P(arena.ptr("s")),
                                               rep) == msm_pkg.INPUT_ERROR
            arena.unchanged()                                     # a miss: nothing at all is written
        with HostArena() as arena:                                 # in place: the only writable bytes are the column itself
            arena.add("io", data=data)
            arena.add("s", 32 * n)
            arena.commit()
            assert L.msm_amd_fr_lookup_permute(cfg.h, h.h, layout, P(arena.ptr("io")), n, 1, P(arena.ptr("io")), P(arena.ptr("s")),
                                               rep) == msm_pkg.OK
            arena.verify()
            assert arena.get("io") == exp_a and arena.get("s") == exp_s
    finally:
        h.free()


# ---- 11. the product column closes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_the_product_closes(cfg, msm_pkg, layout):
    rng = random.Random(77)
    n = 321
    table = lr.random_table(9, n, layout, distinct=250)
    data = pr.column("half", 4, table, layout, n)
    h = cfg.fr_lookup_build(table, layout)
    try:
        a, s, _ = cfg.fr_lookup_permute(h, data, layout)
        pr.check_halo2(data, table, a, s, layout)
        for _ in range(3):
            assert pr.product_closes(data, table, a, s, layout, rng.randrange(R), rng.randrange(R))
        assert not pr.product_closes(data, table, a, s[:32] + s[:32] + s[64:], layout, 5, 7)   # one row of S' lost: it does not
    finally:
        h.free()
