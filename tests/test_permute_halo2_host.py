"""The host twin of the permuted lookup columns in a chosen arrangement (msm_amd_host_fr_lookup_permute_as) on the CPU.
MSM_AMD_PERMUTE_HALO2 against the literal model of upstream's permute_expression_pair in tests/permute_halo2_ref.py (the
twin reduces it to the row-order pipeline over the sorted table; the model does not), MSM_AMD_PERMUTE_ROWS against the twin
and the model of msm_amd_fr_lookup_permute.  Every comparison is of bytes, every output also passes check_halo2, outputs
start as 0xFF bytes.  tests/test_gpu_permute_halo2.py pins the device calls to the twin and the model."""
import ctypes
import os
import random

import pytest

import lookup_ref as lr
import permute_halo2_ref as hr
import permute_ref as pr

R = pr.R
FF = b"\xFF"
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]


def prefilled(nbytes):
    return ctypes.create_string_buffer(FF * nbytes, nbytes)


def agree(msm_pkg, table, data, layout, n_vec=1, threads=0, tag=None):
    """twin(HALO2) = the literal model, for A' and S' together into prefilled buffers and each alone"""
    exp_a, exp_s, exp_rep = hr.permute(table, data, layout, n_vec)
    src, a, s = ctypes.create_string_buffer(data, len(data)), prefilled(len(data)), prefilled(len(data))
    assert msm_pkg.host_fr_lookup_permute_as(table, src, hr.HALO2, layout, n_vec, threads, a_out=a, s_out=s) == (None, None, exp_rep), tag
    assert pr.first_difference(a.raw, exp_a) is None and pr.first_difference(s.raw, exp_s) is None, tag
    assert src.raw == data, tag
    pr.check_halo2(data, table, exp_a, exp_s, layout, n_vec)
    assert msm_pkg.host_fr_lookup_permute_as(table, data, hr.HALO2, layout, n_vec, threads, want_s=False) == (exp_a, None, exp_rep), tag
    assert msm_pkg.host_fr_lookup_permute_as(table, data, hr.HALO2, layout, n_vec, threads, want_a=False) == (None, exp_s, exp_rep), tag
    return exp_a, exp_s, exp_rep


@pytest.mark.parametrize("layout", pr.LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(msm_pkg, n, layout):
    table = lr.random_table(n, n, layout, distinct=max(1, n - n // 4))            # duplicate rows
    for kind in ("uniform", "half", "shuffle"):
        agree(msm_pkg, table, pr.column(kind, n + 1, table, layout, n), layout, tag=(n, kind))


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_one_row_skew_and_no_repeats(msm_pkg, layout):
    n = 300
    table = lr.random_table(7, n, layout)
    rows = pr.decode(table, layout)
    for j in (0, n - 1, 150):
        a, s, rep = agree(msm_pkg, table, pr.column("row%d" % j, 1, table, layout, n), layout, tag=j)
        others = sorted(rows[:j] + rows[j + 1:], reverse=True)
        assert pr.decode(a, layout) == [rows[j]] * n and pr.decode(s, layout) == [rows[j]] + others   # then descending
        assert rep == dict(n_missing=0, first_missing=pr.NO_MISS, rows_hit=1, max_multiplicity=n)
    a, s, rep = agree(msm_pkg, table, pr.column("shuffle", 2, table, layout, n), layout, tag="shuffle")
    assert a == s == pr.encode(sorted(rows), layout)                               # every position is a head


def test_columns_and_threads(msm_pkg):
    layout, n = pr.MONT_LE, 257
    table = lr.random_table(n, n, layout, distinct=n - 9)
    cols = b"".join(pr.column(kind, k, table, layout, n) for k, kind in enumerate(("uniform", "row%d" % (n - 1), "shuffle")))
    for threads in (1, 3, 16):
        agree(msm_pkg, table, cols, layout, 3, threads, tag=threads)


@pytest.mark.parametrize("layout", pr.LAYOUTS)
def test_rows_equal_mod_r(msm_pkg, layout):
    table = lr.edge_records(layout) + pr.encode([5, 7], layout)
    vals = pr.decode(table, layout)
    data = pr.raw([R, 0, R + 5, 5]) + pr.encode([vals[1], vals[1], vals[7], vals[5]], layout)
    agree(msm_pkg, table, data, layout, tag="edge")


def test_known_answer(msm_pkg):
    for case in hr.known()["cases"]:
        assert hr.permute_values(case["A"], case["S"]) == (case["A_perm"], case["S_perm"])
        for layout in pr.LAYOUTS:
            a, s, _ = msm_pkg.host_fr_lookup_permute_as(pr.encode(case["S"], layout), pr.encode(case["A"], layout), hr.HALO2, layout)
            assert (a, s) == (pr.encode(case["A_perm"], layout), pr.encode(case["S_perm"], layout)), case


def test_rows_arrangement_is_the_old_call(msm_pkg):
    for layout in pr.LAYOUTS:
        table = lr.random_table(5, 257, layout, distinct=200)
        cols = b"".join(pr.column(kind, k, table, layout, 257) for k, kind in enumerate(("half", "uniform")))
        exp = pr.permute(table, cols, layout, 2)
        assert msm_pkg.host_fr_lookup_permute_as(table, cols, hr.ROWS, layout, 2) == exp
        assert msm_pkg.host_fr_lookup_permute(table, cols, layout, 2) == exp
        # the two arrangements over the SORTED table: the same A', the same heads
        st = msm_pkg.host_fr_sort(table, layout)[0]
        rows_a, rows_s, _ = msm_pkg.host_fr_lookup_permute_as(st, cols, hr.ROWS, layout, 2)
        h2_a, h2_s, _ = msm_pkg.host_fr_lookup_permute_as(table, cols, hr.HALO2, layout, 2)
        assert rows_a == h2_a and rows_s != h2_s
        A = pr.decode(h2_a, layout)
        for p in range(len(A)):
            if p % 257 == 0 or A[p] != A[p - 1]:
                assert rows_s[32 * p:32 * p + 32] == h2_s[32 * p:32 * p + 32] == h2_a[32 * p:32 * p + 32]


@pytest.mark.parametrize("miss_at", [(4,), (0, 64, 129, 194)])
def test_misses(msm_pkg, miss_at):
    layout, n, n_vec = pr.CANON_LE, 65, 3
    table = lr.random_table(3, n, layout, distinct=40)
    data = lr.draws(11, table, layout, n * n_vec, miss_at)
    assert hr.permute(table, data, layout, n_vec)[:2] == (None, None)
    exp_rep = pr.permute(table, data, layout, n_vec)[2]
    a, s = prefilled(len(data)), prefilled(len(data))
    with pytest.raises(msm_pkg.MsmError) as e:
        msm_pkg.host_fr_lookup_permute_as(table, data, hr.HALO2, layout, n_vec, a_out=a, s_out=s)
    assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep
    assert a.raw == s.raw == FF * len(data)


def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    layout = pr.MONT_LE
    table, data = pr.encode([5, 1, 2, 7, 1][:4], layout), pr.encode([1, 1, 2, 7], layout)
    a, s = ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(32 * 4)
    rep = (ctypes.c_uint64 * 4)()
    big = ctypes.create_string_buffer(32 * 16)
    at = ctypes.addressof(big)
    P = ctypes.c_void_p
    good = dict(layout=layout, how=hr.HALO2, table=table, n_rows=4, data=data, n=4, n_vec=1, threads=0, a=a, s=s, rep=rep)

    def call(**kw):
        x = dict(good, **kw)
        return L.msm_amd_host_fr_lookup_permute_as(x["layout"], x["how"], x["table"], x["n_rows"], x["data"], x["n"], x["n_vec"],
                                                   x["threads"], x["a"], x["s"], x["rep"])
    assert call() == msm_pkg.OK and list(rep) == [0, pr.NO_MISS, 3, 2]
    assert (a.raw, s.raw) == (pr.encode([1, 1, 2, 7], layout), pr.encode([1, 5, 2, 7], layout))
    assert call(how=hr.ROWS) == msm_pkg.OK and call(a=None) == msm_pkg.OK and call(s=None, n=3) == msm_pkg.OK
    errors = dict(unknown_arrangement=dict(how=2), negative_arrangement=dict(how=-1),
                  unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), null_table=dict(table=None), no_rows=dict(n_rows=0),
                  rows_2_31=dict(n_rows=1 << 31), null_in=dict(data=None), null_report=dict(rep=None),
                  no_output=dict(a=None, s=None), s_with_other_n=dict(n=3),
                  n_2_32=dict(n=1 << 32, s=None), product_2_32=dict(n=1 << 16, n_vec=1 << 16, s=None),
                  a_over_in=dict(data=P(at), a=P(at + 32 * 3)), s_is_in=dict(data=P(at), s=P(at)),
                  s_over_a=dict(a=P(at), s=P(at + 32 * 3)))
    for name, kw in errors.items():
        assert call(**kw) == msm_pkg.INPUT_ERROR, name
    assert call(data=None, n=0) == msm_pkg.OK and list(rep) == [0, 0, 0, 0]


def test_model_self_check_the_reduction_is_the_literal_algorithm():
    """A self-check of the two models; it calls nothing in the library.  The row-order definition over the sorted table with
    the gaps taken from the far end IS permute_expression_pair: 20 000 random small cases with duplicate rows, big integers only"""
    rng = random.Random(2025)
    for case in range(20000):
        n = rng.randrange(1, 12)
        pool = [rng.randrange(8) for _ in range(rng.randrange(1, n + 1))]
        S = [rng.choice(pool) for _ in range(n)]
        A = [rng.choice(S) for _ in range(n)]
        T = sorted(S)
        first = {}
        for k, x in enumerate(T):
            first.setdefault(x, k)
        c = [0] * n
        for x in A:
            c[first[x]] += 1
        U = [k for k in range(n) if c[k] == 0]
        a, s, g = [], [], 0
        for k in range(n):
            for rank in range(c[k]):
                a.append(T[k])
                if rank == 0:
                    s.append(T[k])
                else:
                    s.append(T[U[len(U) - 1 - g]])
                    g += 1
        assert (a, s) == hr.permute_values(A, S), (A, S)


def test_exports(msm_pkg):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msm_amd.h")).read()
    for name in ("msm_amd_fr_lookup_build_sorted", "msm_amd_fr_lookup_sorted", "msm_amd_fr_lookup_permute_as",
                 "msm_amd_host_fr_lookup_permute_as"):
        assert name in msm_pkg.EXPORTS and ("int %s(" % name) in header
        assert getattr(msm_pkg.lib(), name)
    assert "MSM_AMD_PERMUTE_ROWS = 0, MSM_AMD_PERMUTE_HALO2 = 1" in header
    assert "NOT confirmed against a halo2 build" in header
    assert (msm_pkg.PERMUTE_ROWS, msm_pkg.PERMUTE_HALO2) == (hr.ROWS, hr.HALO2)
