"""The permuted lookup columns in a chosen arrangement on the GPU (msm_amd_fr_lookup_build_sorted, msm_amd_fr_lookup_permute_as)
against the host twin and the literal model of upstream's permute_expression_pair in tests/permute_halo2_ref.py
(tests/test_permute_halo2_host.py pins the twin to the model on the CPU).  Every comparison is of bytes: ctx call = twin =
model for both `mem` forms, over a sorted handle built from host rows and one built from device rows, into buffers that
start as 0xFF bytes; the inputs of an out-of-place call are as they were afterwards; every output passes check_halo2.  The
knobs of tests/test_gpu_permute.py reach the same kernels here.  The device form writes the caller's buffers from the fill
kernel itself, so the guard bands and the miss cases here see what the host form's staging hides."""
import ctypes

import pytest

import lookup_ref as lr
import permute_halo2_ref as hr
import permute_ref as pr
import sort_ref as sr
from guard import Arena

pytestmark = pytest.mark.gpu

R = pr.R
FF = b"\xFF"
HOST, DEVICE = sr.MEM_HOST, sr.MEM_DEVICE


def prefilled(nbytes):
    return ctypes.create_string_buffer(FF * nbytes, nbytes)


def sorted_handles(cfg, table, layout):
    """a sorted handle built from host rows and one built from device rows, which are overwritten afterwards; both with the
    permutation, which must be the stable sort permutation of the table"""
    n_rows = len(table) // 32
    exp_perm = sr.sort(table, layout)[1]
    h0, perm = cfg.fr_lookup_build_sorted(table, layout)
    assert perm == exp_perm
    d_table, d_perm = cfg.alloc(max(32, len(table))), cfg.alloc(4 * n_rows)
    try:
        cfg.to_device(d_table, table)
        cfg.to_device(d_perm, FF * 4 * n_rows)
        h1, _ = cfg.fr_lookup_build_sorted(d_table, layout, n_rows, DEVICE, perm_out=d_perm)
        back = cfg.to_host(d_perm, 4 * n_rows)
        assert [int.from_bytes(back[i:i + 4], "little") for i in range(0, len(back), 4)] == exp_perm
        assert cfg.to_host(d_table, len(table)) == table
        cfg.to_device(d_table, b"\xEE" * len(table))
    finally:
        cfg.free(d_table)
        cfg.free(d_perm)
    assert cfg.fr_lookup_sorted(h0) and cfg.fr_lookup_sorted(h1)
    return [h0, h1]


def device_permute(cfg, h, data, how, layout, n_vec, want_a=True, want_s=True, in_place=False):
    """MEM_DEVICE on fresh buffers that start as 0xFF: (A', S', report, the input afterwards); a miss raises"""
    nb = len(data)
    d_in, d_a, d_s = cfg.alloc(nb), cfg.alloc(nb), cfg.alloc(nb)
    try:
        cfg.to_device(d_in, data)
        cfg.to_device(d_a, FF * nb)
        cfg.to_device(d_s, FF * nb)
        err = None
        try:
            _, _, rep = cfg.fr_lookup_permute_as(h, d_in, how, layout, n_vec, DEVICE, n=nb // 32 // n_vec,
                                                 a_out=(d_in if in_place else d_a) if want_a else None, s_out=d_s if want_s else None)
        except Exception as e:                                   # noqa: BLE001 -- handed on once the buffers are read
            err, rep = e, None
        out = (cfg.to_host(d_a, nb), cfg.to_host(d_s, nb), rep, cfg.to_host(d_in, nb))
    finally:
        for p in (d_in, d_a, d_s):
            cfg.free(p)
    if err is not None:
        err.buffers = out
        raise err
    return out


def check(cfg, msm_pkg, table, data, layout, n_vec=1, tag=None):
    """HALO2: ctx call = twin = literal model, both mem forms, both kinds of sorted handle; returns (A', S', report)"""
    exp_a, exp_s, exp_rep = hr.permute(table, data, layout, n_vec)
    assert msm_pkg.host_fr_lookup_permute_as(table, data, hr.HALO2, layout, n_vec) == (exp_a, exp_s, exp_rep), tag
    pr.check_halo2(data, table, exp_a, exp_s, layout, n_vec)
    hs = sorted_handles(cfg, table, layout)
    try:
        for h in hs:
            src, a, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data)), prefilled(len(data))
            assert cfg.fr_lookup_permute_as(h, src, hr.HALO2, layout, n_vec, a_out=a, s_out=s) == (None, None, exp_rep), tag
            assert pr.first_difference(a.raw, exp_a) is None, (tag, "host A'")
            assert pr.first_difference(s.raw, exp_s) is None, (tag, "host S'")
            assert src.raw == data, tag
            d_a, d_s, rep, d_src = device_permute(cfg, h, data, hr.HALO2, layout, n_vec)
            assert pr.first_difference(d_a, exp_a) is None, (tag, "device A'")
            assert pr.first_difference(d_s, exp_s) is None, (tag, "device S'")
            assert rep == exp_rep and d_src == data, tag
        h = hs[0]
        assert cfg.fr_lookup_permute_as(h, data, hr.HALO2, layout, n_vec, want_s=False) == (exp_a, None, exp_rep), tag
        assert cfg.fr_lookup_permute_as(h, data, hr.HALO2, layout, n_vec, want_a=False) == (None, exp_s, exp_rep), tag
        assert device_permute(cfg, h, data, hr.HALO2, layout, n_vec, want_s=False)[:2] == (exp_a, FF * len(data)), tag
        assert device_permute(cfg, h, data, hr.HALO2, layout, n_vec, want_a=False)[:2] == (FF * len(data), exp_s), tag
        assert device_permute(cfg, h, data, hr.HALO2, layout, n_vec, in_place=True)[1::2] == (exp_s, exp_a), tag
    finally:
        for h in hs:
            h.free()
    return exp_a, exp_s, exp_rep


# ---- 1. sizes across the wave and the workgroup; tables with duplicate rows -------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(cfg, msm_pkg, n):
    for layout in pr.LAYOUTS:
        table = lr.random_table(n + layout, n, layout, distinct=max(1, n - n // 4))
        check(cfg, msm_pkg, table, pr.column("uniform", n, table, layout, n), layout, tag=(n, layout))


# ---- 2. plans of three, four and five levels that end in partial tiles; two columns ------------------------------------------------
@pytest.mark.parametrize("n,levels", [(17, 3), (65, 4), (300, 5)])
def test_many_level_plans(cfg, msm_pkg, n, levels, monkeypatch):
    layout = pr.CANON_LE
    table = lr.random_table(n, n, layout, distinct=n - n // 3)
    cols = b"".join(pr.column(kind, n + k, table, layout, n) for k, kind in enumerate(("uniform", "half")))
    default = check(cfg, msm_pkg, table, cols, layout, 2, tag=(n, "default"))
    monkeypatch.setenv("MSM_AMD_PERMUTE_TILE_LOG", "2")
    assert msm_pkg.test_fr_permute_plan(n, 2, 2)["levels"] == levels
    assert check(cfg, msm_pkg, table, cols, layout, 2, tag=(n, "tiles of 4")) == default


# ---- 3. skew: one row takes every input; no repeats: every position is a head -----------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_skew_and_no_repeats(cfg, msm_pkg, layout):
    n = 513
    table = lr.random_table(31, n, layout)
    rows = pr.decode(table, layout)
    for j in (0, n - 1, 350):
        a, s, rep = check(cfg, msm_pkg, table, pr.column("row%d" % j, 1, table, layout, n), layout, tag=j)
        assert pr.decode(a, layout) == [rows[j]] * n
        assert pr.decode(s, layout) == [rows[j]] + sorted(rows[:j] + rows[j + 1:], reverse=True)   # then all others DEscending
        assert rep == dict(n_missing=0, first_missing=pr.NO_MISS, rows_hit=1, max_multiplicity=n)
    a, s, rep = check(cfg, msm_pkg, table, pr.column("half", 2, table, layout, n), layout, tag="half")
    assert rep["max_multiplicity"] >= n // 2
    a, s, rep = check(cfg, msm_pkg, table, pr.column("shuffle", 3, table, layout, n), layout, tag="shuffle")
    assert a == s == pr.encode(sorted(rows), layout) and rep["rows_hit"] == n and rep["max_multiplicity"] == 1


# ---- 4. both fill forms, long and short tiles, three columns ----------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["search", "scan"])
@pytest.mark.parametrize("tile_log", ["11", "2"])
def test_fill_forms_give_the_same_bytes(cfg, msm_pkg, tile_log, fill, monkeypatch):
    layout = pr.CANON_LE
    table = lr.random_table(47, 300, layout, distinct=211)
    cols = b"".join(pr.column(kind, k, table, layout, 300) for k, kind in enumerate(("half", "row299", "shuffle")))
    monkeypatch.setenv("MSM_AMD_PERMUTE_TILE_LOG", tile_log)
    monkeypatch.setenv("MSM_AMD_PERMUTE_FILL", fill)
    check(cfg, msm_pkg, table, cols, layout, 3, tag=(fill, tile_log))


# ---- 5. rows equal mod r under different words; the known answer ------------------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_rows_equal_mod_r_and_known_answer(cfg, msm_pkg, layout):
    table = lr.edge_records(layout) + pr.encode([5, 7], layout)
    vals = pr.decode(table, layout)
    data = pr.raw([R, 0, R + 5, 5]) + pr.encode([vals[1], vals[1], vals[7], vals[5]], layout)
    check(cfg, msm_pkg, table, data, layout, tag="edge")
    for case in hr.known()["cases"]:
        a, s, _ = check(cfg, msm_pkg, pr.encode(case["S"], layout), pr.encode(case["A"], layout), layout, tag="known")
        assert (a, s) == (pr.encode(case["A_perm"], layout), pr.encode(case["S_perm"], layout))


# ---- 6. cross-checks between the arrangements, the handles and the calls -----------------------------------------------------------
@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_cross_checks(cfg, msm_pkg, layout):
    n, n_vec = 257, 2
    table = lr.random_table(5, n, layout, distinct=200)
    cols = b"".join(pr.column(kind, k, table, layout, n) for k, kind in enumerate(("half", "uniform")))
    plain = cfg.fr_lookup_build(table, layout)
    hs = sorted_handles(cfg, table, layout)
    try:
        assert not cfg.fr_lookup_sorted(plain)
        # ROWS on a plain handle is msm_amd_fr_lookup_permute, for both mem forms
        old = cfg.fr_lookup_permute(plain, cols, layout, n_vec)
        assert old == pr.permute(table, cols, layout, n_vec)
        assert cfg.fr_lookup_permute_as(plain, cols, hr.ROWS, layout, n_vec) == old
        d_a, d_s, rep, d_src = device_permute(cfg, plain, cols, hr.ROWS, layout, n_vec)
        assert (d_a, d_s, rep) == old and d_src == cols
        # ROWS and HALO2 on a sorted handle: the same A'; ROWS there is the row-order definition over the sorted table
        sorted_table, perm = sr.sort(table, layout)
        for h in hs:
            rows_a, rows_s, _ = cfg.fr_lookup_permute_as(h, cols, hr.ROWS, layout, n_vec)
            h2_a, h2_s, _ = cfg.fr_lookup_permute_as(h, cols, hr.HALO2, layout, n_vec)
            assert rows_a == h2_a and (rows_a, rows_s) == pr.permute(sorted_table, cols, layout, n_vec)[:2] and rows_s != h2_s
            # multiplicities on the sorted handle credit positions: m_sorted[k] == m_plain[perm[k]]
            m_plain = cfg.fr_lookup_multiplicities(plain, cols, scalar_layout=layout, n_vec=n_vec)[0]
            m_sorted = cfg.fr_lookup_multiplicities(h, cols, scalar_layout=layout, n_vec=n_vec)[0]
            assert m_sorted == b"".join(m_plain[32 * p:32 * p + 32] for p in perm)
            assert m_sorted == lr.multiplicities(sorted_table, cols, layout)[0]
            assert cfg.fr_lookup_info(h)["n_distinct"] == 200
    finally:
        for h in hs + [plain]:
            h.free()


# ---- 7. failures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss_at", [(4,), (0, 64, 129, 194)])
def test_misses(cfg, msm_pkg, miss_at):
    layout, n, n_vec = pr.CANON_LE, 65, 3
    table = lr.random_table(3, n, layout, distinct=40)
    data = lr.draws(11, table, layout, n * n_vec, miss_at)
    exp_rep = pr.permute(table, data, layout, n_vec)[2]
    assert exp_rep["n_missing"] == len(miss_at) and exp_rep["first_missing"] == miss_at[0]
    hs = sorted_handles(cfg, table, layout)
    try:
        for h in hs:
            for how in (hr.ROWS, hr.HALO2):
                src, a, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data)), prefilled(len(data))
                with pytest.raises(msm_pkg.MsmError) as e:
                    cfg.fr_lookup_permute_as(h, src, how, layout, n_vec, a_out=a, s_out=s)
                assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep
                assert a.raw == s.raw == FF * len(data) and src.raw == data
                with pytest.raises(msm_pkg.MsmError) as e:           # the fill kernel itself obeys the miss counter
                    device_permute(cfg, h, data, how, layout, n_vec)
                assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep
                assert e.value.buffers == (FF * len(data), FF * len(data), None, data)
                with pytest.raises(msm_pkg.MsmError) as e:           # in place: the inputs stay
                    device_permute(cfg, h, data, how, layout, n_vec, in_place=True)
                assert e.value.buffers[3] == data and e.value.buffers[1] == FF * len(data)
    finally:
        for h in hs:
            h.free()


def test_argument_errors(cfg, msm_pkg):
    L = msm_pkg.lib()
    layout, n = pr.MONT_LE, 64
    table = lr.random_table(3, n, layout)
    data = pr.column("uniform", 1, table, layout, n)
    plain = cfg.fr_lookup_build(table, layout)
    h, _ = cfg.fr_lookup_build_sorted(table, layout)
    d = cfg.alloc(32 * n * 4)
    big = ctypes.create_string_buffer(data + FF * (32 * n * 3), 32 * n * 4)
    rep = (ctypes.c_uint64 * 4)()
    P = ctypes.c_void_p
    try:
        cfg.to_device(d, big.raw)
        image, image_bytes = cfg.test_fr_lookup_image(h), cfg.fr_lookup_info(h)["device_bytes"]
        for mem, at in ((DEVICE, d), (HOST, ctypes.addressof(big))):
            good = dict(h=h.h, mem=mem, layout=layout, how=hr.HALO2, src=at, n=n, n_vec=1, a=at + 32 * n, s=at + 64 * n, rep=rep)

            def call(**kw):
                x = dict(good, **kw)
                return L.msm_amd_fr_lookup_permute_as(cfg.h, x["h"], x["mem"], x["layout"], x["how"], P(x["src"]), x["n"], x["n_vec"],
                                                      P(x["a"]), P(x["s"]), x["rep"], None)
            errors = dict(plain_handle=dict(h=plain.h), unknown_mem=dict(mem=2), unknown_arrangement=dict(how=2),
                          unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), null_in=dict(src=None), null_report=dict(rep=None),
                          no_output=dict(a=None, s=None), s_with_other_n=dict(n=63), foreign_handle=dict(h=P(at)),
                          a_over_in=dict(a=at + 32), s_is_in=dict(s=at), s_over_a=dict(s=at + 32 * n + 32 * 63),
                          n_2_32=dict(n=1 << 32, s=None), product_2_32=dict(n=1 << 16, n_vec=1 << 16, s=None))
            if mem == DEVICE:
                errors.update(misaligned_in=dict(src=at + 8), misaligned_a=dict(a=at + 32 * n + 4), misaligned_s=dict(s=at + 64 * n + 8),
                              a_in_image=dict(a=image), s_over_image_end=dict(s=image + image_bytes - 32),
                              in_in_image=dict(src=image + 32, s=None), a_ends_in_image=dict(a=image - 32 * n + 32))
            for name, kw in errors.items():
                assert call(**kw) == msm_pkg.INPUT_ERROR, (mem, name)
                assert b"msm_amd_fr_lookup_permute_as" in L.msm_amd_last_error(cfg.h), name
            assert cfg.to_host(d, 32 * n * 4) == big.raw == data + FF * (32 * n * 3), mem     # the refused calls wrote nothing
        assert L.msm_amd_fr_lookup_permute_as(cfg.h, plain.h, DEVICE, layout, hr.ROWS, P(d), n, 1, P(d + 32 * n), P(d + 64 * n), rep,
                                              None) == msm_pkg.OK                                   # ROWS takes any handle
        flag = ctypes.c_int(7)
        assert L.msm_amd_fr_lookup_sorted(cfg.h, P(ctypes.addressof(big)), flag) == msm_pkg.INPUT_ERROR and flag.value == 7
        assert L.msm_amd_fr_lookup_sorted(cfg.h, h.h, None) == msm_pkg.INPUT_ERROR
        out = ctypes.c_void_p()
        for kw in (dict(mem=2), dict(layout=msm_pkg.SCALAR_CANON_BE32), dict(table=None), dict(n_rows=0), dict(n_rows=1 << 31),
                   dict(mem=DEVICE, table=P(d + 8)), dict(mem=DEVICE, table=P(d), perm=P(d + 32 * n + 2)),
                   dict(mem=DEVICE, table=P(d), perm=P(d + 64)), dict(perm=P(ctypes.addressof(big) + 4))):
            x = dict(dict(mem=HOST, layout=layout, table=P(ctypes.addressof(big)), n_rows=n, perm=None), **kw)
            assert L.msm_amd_fr_lookup_build_sorted(cfg.h, x["mem"], x["layout"], x["table"], x["n_rows"], x["perm"], ctypes.byref(out),
                                                    None) == msm_pkg.INPUT_ERROR, kw
            assert out.value is None
    finally:
        cfg.free(d)
        plain.free()
        h.free()


# ---- 8. guard bands round a_out and s_out on device buffers; a miss writes nothing at all ------------------------------------------
@pytest.mark.parametrize("how", [hr.ROWS, hr.HALO2])
def test_guard_bands(cfg, msm_pkg, how):
    L = msm_pkg.lib()
    P = ctypes.c_void_p
    layout, n = pr.MONT_LE, 257
    table = lr.random_table(n, n, layout, distinct=n - 20)
    data = pr.column("half", n, table, layout, n)
    h, perm = cfg.fr_lookup_build_sorted(table, layout)
    exp_a, exp_s, exp_rep = hr.permute(table, data, layout) if how == hr.HALO2 else pr.permute(sr.sort(table, layout)[0], data, layout)
    rep = (ctypes.c_uint64 * 4)()

    def call(arena, src, a, s):
        return L.msm_amd_fr_lookup_permute_as(cfg.h, h.h, DEVICE, layout, how, P(arena.ptr(src)), n, 1, P(arena.ptr(a)),
                                              P(arena.ptr(s)), rep, None)
    try:
        with Arena(cfg) as arena:
            arena.add("in", data=data, readonly=True)
            arena.add("a", 32 * n)
            arena.add("s", 32 * n)
            arena.commit()
            assert call(arena, "in", "a", "s") == msm_pkg.OK
            arena.verify()
            assert dict(zip(msm_pkg.LOOKUP_REPORT_FIELDS, rep)) == exp_rep and arena.get("a") == exp_a and arena.get("s") == exp_s
            arena.set("in", lr.draws(5, table, layout, n, (n - 1,)))
            arena.commit()
            assert call(arena, "in", "a", "s") == msm_pkg.INPUT_ERROR
            arena.unchanged()                                     # a miss: the fill kernel stores nothing
        with Arena(cfg) as arena:                                  # in place: the only writable bytes are the column itself
            arena.add("io", data=data)
            arena.add("s", 32 * n)
            arena.commit()
            assert call(arena, "io", "io", "s") == msm_pkg.OK
            arena.verify()
            assert arena.get("io") == exp_a and arena.get("s") == exp_s
        with Arena(cfg) as arena:                                  # build_sorted on device buffers: the table is read-only
            arena.add("table", data=table, readonly=True)
            arena.add("perm", 4 * n)
            arena.commit()
            out = ctypes.c_void_p()
            assert L.msm_amd_fr_lookup_build_sorted(cfg.h, DEVICE, layout, P(arena.ptr("table")), n, P(arena.ptr("perm")),
                                                    ctypes.byref(out), None) == msm_pkg.OK
            arena.verify()
            back = arena.get("perm")
            assert [int.from_bytes(back[i:i + 4], "little") for i in range(0, len(back), 4)] == perm
            assert L.msm_amd_fr_lookup_free(cfg.h, out) == msm_pkg.OK
    finally:
        h.free()
