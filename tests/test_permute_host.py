"""The host twin of halo2's permuted lookup columns (msm_amd_host_fr_lookup_permute) and the pure plan tap against the
big-integer model of tests/permute_ref.py, on the CPU.  Every comparison is of bytes, and every output also has to pass
check_halo2, which tests the constraints of the lookup argument without the model.  tests/test_gpu_permute.py pins the
device calls to the twin and the model."""
import ctypes
import random

import pytest

import lookup_ref as lr
import permute_ref as pr

R = pr.R
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def agree(msm_pkg, table, data, layout, n_vec=1, threads=0, tag=None):
    """twin = model for A' and S' together, each alone, and halo2's constraints on the result"""
    exp_a, exp_s, exp_rep = pr.permute(table, data, layout, n_vec)
    a, s, rep = msm_pkg.host_fr_lookup_permute(table, data, layout, n_vec, threads)
    assert pr.first_difference(a, exp_a) is None and pr.first_difference(s, exp_s) is None, tag
    assert rep == exp_rep, (tag, rep, exp_rep)
    pr.check_halo2(data, table, a, s, layout, n_vec)
    assert msm_pkg.host_fr_lookup_permute(table, data, layout, n_vec, threads, want_s=False) == (exp_a, None, exp_rep), tag
    assert msm_pkg.host_fr_lookup_permute(table, data, layout, n_vec, threads, want_a=False) == (None, exp_s, exp_rep), tag
    return a, s, rep


@pytest.mark.parametrize("layout", pr.LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(msm_pkg, n, layout):
    table = lr.random_table(n, n, layout, distinct=max(1, n - n // 4))
    for kind in ("uniform", "half", "shuffle"):
        agree(msm_pkg, table, pr.column(kind, n + 1, table, layout, n), layout, tag=(n, kind))


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_skew_and_no_repeats(msm_pkg, layout):
    n = 300
    table = lr.random_table(7, n, layout)
    rows = pr.decode(table, layout)
    for j in (0, n - 1, 150):
        a, s, rep = agree(msm_pkg, table, pr.column("row%d" % j, 1, table, layout, n), layout, tag=j)
        assert pr.decode(a, layout) == [rows[j]] * n
        assert pr.decode(s, layout) == [rows[j]] + rows[:j] + rows[j + 1:]     # the row, then all others ascending
        assert rep == dict(n_missing=0, first_missing=pr.NO_MISS, rows_hit=1, max_multiplicity=n)
    a, s, rep = agree(msm_pkg, table, pr.column("shuffle", 2, table, layout, n), layout, tag="shuffle")
    assert a == s == table and rep["rows_hit"] == n and rep["max_multiplicity"] == 1   # every position is a head


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_rows_equal_mod_r(msm_pkg, layout):
    """r beside 0 and r + 5 beside 5 as words of the table: the representative is the smaller index, the duplicate leaves
    through the unused rows, and every output record is reduced"""
    table = lr.edge_records(layout) + pr.encode([5, 7], layout)          # 0 1 r-1 r r+5 2^256-1 5 7 as words
    vals = pr.decode(table, layout)
    data = pr.raw([R, 0, R + 5, 5]) + pr.encode([vals[1], vals[1], vals[7], vals[5]], layout)
    a, s, rep = agree(msm_pkg, table, data, layout, tag="edge")
    assert pr.decode(a, layout)[:2] == [vals[0], vals[0]] and rep["n_missing"] == 0
    assert pr.decode(s, layout)[1] == vals[2]                             # the first unused row: word r - 1
    agree(msm_pkg, pr.raw([R + 5, 5, R, 0]), pr.raw([5, 0, R + 5, 2 * R]), layout, tag="r + 5 beside 5")


@pytest.mark.parametrize("layout", pr.LAYOUTS)
@pytest.mark.parametrize("n", [65, 257])
def test_several_columns(msm_pkg, n, layout):
    table = lr.random_table(n, n, layout, distinct=n - 9)
    cols = [pr.column(kind, k, table, layout, n) for k, kind in enumerate(("uniform", "row%d" % (n - 1), "shuffle"))]
    a, s, rep = agree(msm_pkg, table, b"".join(cols), layout, 3, tag=n)
    for k, col in enumerate(cols):                                        # no counter of a column leaks into the next
        one = msm_pkg.host_fr_lookup_permute(table, col, layout)
        assert (a[32 * n * k:32 * n * (k + 1)], s[32 * n * k:32 * n * (k + 1)]) == one[:2], (n, k)


def test_output_combinations_threads_and_empty(msm_pkg):
    layout = pr.MONT_LE
    table = lr.random_table(3, 100, layout, distinct=60)
    for n in (7, 100, 333):                                               # a_out alone: any n
        data = pr.column("uniform", n, table, layout, n)
        exp_a, _, exp_rep = pr.permute(table, data, layout, want_s=False)
        for threads in (1, 3, 16):
            assert msm_pkg.host_fr_lookup_permute(table, data, layout, 1, threads, want_s=False) == (exp_a, None, exp_rep)
        buf = ctypes.create_string_buffer(data, len(data))                # in place
        rep = (ctypes.c_uint64 * 4)()
        assert msm_pkg.lib().msm_amd_host_fr_lookup_permute(layout, table, 100, buf, n, 1, 3, buf, None, rep) == msm_pkg.OK
        assert buf.raw == exp_a
    for n_vec in (1, 0):
        assert msm_pkg.host_fr_lookup_permute(table, b"", layout, n_vec) == (b"", b"", dict.fromkeys(msm_pkg.LOOKUP_REPORT_FIELDS, 0))


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_a_miss_leaves_the_outputs(msm_pkg, layout):
    n = 65
    table = lr.random_table(3, n, layout, distinct=40)
    for n_vec, miss_at in ((1, (64,)), (3, (4,)), (3, (100,)), (3, (194,)), (3, (4, 100, 194)), (1, tuple(range(n)))):
        data = lr.draws(11, table, layout, n * n_vec, miss_at)
        _, _, exp_rep = pr.permute(table, data, layout, n_vec)
        assert exp_rep["n_missing"] == len(miss_at) and exp_rep["first_missing"] == miss_at[0]
        a = ctypes.create_string_buffer(b"\xFF" * (32 * n * n_vec), 32 * n * n_vec)
        s = ctypes.create_string_buffer(b"\xFF" * (32 * n * n_vec), 32 * n * n_vec)
        with pytest.raises(msm_pkg.MsmError) as e:
            msm_pkg.host_fr_lookup_permute(table, data, layout, n_vec, a_out=a, s_out=s)
        assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep, (miss_at, e.value.report, exp_rep)
        assert a.raw == s.raw == b"\xFF" * (32 * n * n_vec)              # untouched


@pytest.mark.parametrize("n_rows", [1, 2, 17, 65, 300, 2048, 2049, (1 << 22) + 1, (1 << 31) - 1])
def test_plan_tap(msm_pkg, n_rows):
    for tile_log in range(2, pr.DEFAULT_TILE_LOG + 1):
        for n_vec in (1, 2, 3):
            if n_rows * n_vec >> 32:
                continue
            assert msm_pkg.test_fr_permute_plan(n_rows, n_vec, tile_log) == pr.plan(n_rows, n_vec, tile_log), (n_vec, tile_log)
    assert [msm_pkg.test_fr_permute_plan(n, 1, 2)["levels"] for n in (17, 65, 300)] == [3, 4, 5]
    for bad in ((0, 1, 11), (5, 0, 11), (1 << 31, 1, 11), (1 << 30, 4, 11), (5, 1, 1), (5, 1, 12)):
        with pytest.raises(msm_pkg.MsmError):
            msm_pkg.test_fr_permute_plan(*bad)


def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    layout = pr.MONT_LE
    table, data = pr.encode([1, 2, 3, 4], layout), pr.encode([1, 1, 2, 4], layout)
    a, s = ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(32 * 4)
    rep = (ctypes.c_uint64 * 4)()
    big = ctypes.create_string_buffer(32 * 16)
    at = ctypes.addressof(big)
    P = ctypes.c_void_p
    good = dict(layout=layout, table=table, n_rows=4, data=data, n=4, n_vec=1, threads=0, a=a, s=s, rep=rep)

    def call(**kw):
        x = dict(good, **kw)
        return L.msm_amd_host_fr_lookup_permute(x["layout"], x["table"], x["n_rows"], x["data"], x["n"], x["n_vec"], x["threads"],
                                                x["a"], x["s"], x["rep"])
    assert call() == msm_pkg.OK and list(rep) == [0, pr.NO_MISS, 3, 2]
    assert call(a=None) == msm_pkg.OK and call(s=None) == msm_pkg.OK
    assert call(s=None, n=3) == msm_pkg.OK                                # without s_out any n goes
    errors = dict(unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), null_table=dict(table=None), no_rows=dict(n_rows=0),
                  rows_2_31=dict(n_rows=1 << 31), null_in=dict(data=None), null_report=dict(rep=None),
                  no_output=dict(a=None, s=None), s_with_other_n=dict(n=3), s_with_larger_n=dict(n_rows=3),
                  n_2_32=dict(n=1 << 32, s=None), product_2_32=dict(n=1 << 16, n_vec=1 << 16, s=None),
                  a_over_in=dict(data=P(at), a=P(at + 32 * 3)), a_under_in=dict(data=P(at + 32), a=P(at)),
                  s_is_in=dict(data=P(at), s=P(at)), s_over_in=dict(data=P(at), s=P(at + 32 * 3)),
                  s_is_a=dict(a=P(at), s=P(at)), s_over_a=dict(a=P(at), s=P(at + 32 * 3)))
    for name, kw in errors.items():
        assert call(**kw) == msm_pkg.INPUT_ERROR, name
    assert call(data=None, n=0) == msm_pkg.OK and call(data=None, n_vec=0) == msm_pkg.OK and list(rep) == [0, 0, 0, 0]
    assert call(data=None, n=0, rep=None) == msm_pkg.INPUT_ERROR and call(n=0, a=None, s=None) == msm_pkg.INPUT_ERROR
    ctypes.memmove(at, data, len(data))
    assert call(data=P(at), a=P(at), s=P(at + 32 * 4)) == msm_pkg.OK      # in place, and adjacent is disjoint
    assert ctypes.string_at(at, 32 * 8) == pr.permute(table, data, layout)[0] + pr.permute(table, data, layout)[1]


def test_the_model_passes_halo2s_constraints():
    """the definition itself, 2000 random tables with duplicates, n = 1 .. 300: uniform draws, one row n times, a shuffle of
    the table; the product with big integers on every tenth case (a self-check of the model: it calls nothing in the library)"""
    rng = random.Random(2024)
    for case in range(2000):
        n = rng.randrange(1, 301)
        layout = pr.LAYOUTS[case % 2]
        table = lr.random_table(case, n, layout, distinct=rng.randrange(1, n + 1))
        kind = ("uniform", "row%d" % rng.randrange(n), "shuffle")[case % 3]
        data = pr.column(kind, case, table, layout, n)
        a, s, rep = pr.permute(table, data, layout)
        pr.check_halo2(data, table, a, s, layout)
        if case % 10 == 0:
            assert pr.product_closes(data, table, a, s, layout, rng.randrange(R), rng.randrange(R))
