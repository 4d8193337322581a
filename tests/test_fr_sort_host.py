"""The host twin of the sort of Fr records by canonical value (msm_amd_host_fr_sort) and the pure planner aid
(msm_amd_test_fr_sort_plan) against the model of tests/sort_ref.py, on the CPU.  Every comparison is of bytes; outputs start
as 0xFF bytes; the inputs of an out-of-place call are unchanged afterwards.  tests/test_gpu_fr_sort.py pins the device
call to the twin and the model."""
import ctypes
import os
import random

import pytest

import lookup_ref as lr
import sort_ref as sr

R = sr.R
FF = b"\xFF"
MASKS = (0, 1, 0x3, 0x80000000, 0x00020001, 0xFFFFFFFF)


def prefilled(nbytes):
    return ctypes.create_string_buffer(FF * nbytes, nbytes)


def agree(msm_pkg, data, layout, n_vec=1, threads=0, tag=None):
    """twin = model: both outputs together into prefilled buffers, each alone; returns (records, perm)"""
    exp_out, exp_perm = sr.sort(data, layout, n_vec)
    total = len(data) // 32
    src, out = ctypes.create_string_buffer(data, len(data)), prefilled(len(data))
    perm = (ctypes.c_uint32 * max(1, total))(*([0xFFFFFFFF] * max(1, total)))
    assert msm_pkg.host_fr_sort(src, layout, n_vec, threads, n=total // n_vec, out=out, perm_out=perm) == (None, None), tag
    assert sr.first_difference(out.raw, exp_out) is None, tag
    assert list(perm[:total]) == exp_perm, tag
    assert src.raw == data, tag
    assert msm_pkg.host_fr_sort(data, layout, n_vec, threads, want_perm=False) == (exp_out, None), tag
    assert msm_pkg.host_fr_sort(data, layout, n_vec, threads, want_out=False) == (None, exp_perm), tag
    sr.runs_ascend(data, exp_perm, layout, n_vec)
    return exp_out, exp_perm


@pytest.mark.parametrize("layout", sr.LAYOUTS)
@pytest.mark.parametrize("n", sr.SIZES)
def test_sizes(msm_pkg, n, layout):
    agree(msm_pkg, sr.random_column(n + layout, n, layout), layout, tag=(n, layout))


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_threads_do_not_show(msm_pkg, threads):
    for layout in sr.LAYOUTS:
        agree(msm_pkg, sr.few_values(5, 5000, layout, 5), layout, threads=threads, tag=("few", threads))
        agree(msm_pkg, sr.random_column(6, 1025, layout), layout, threads=threads, tag=("random", threads))


def test_records_equal_mod_r(msm_pkg):
    """x, x + r, x + 4 r as words of a CANON_LE column are one value: they keep their input order, and every output record
    is the reduced one; the edge words 0, 1, r - 1, r, r + 5, 2^256 - 1 in both layouts"""
    xs = [5, 0, (1 << 253) + 7, 1]
    ws = [x + k * R for x in xs for k in (4, 1, 0) if x + k * R < (1 << 256)]
    random.Random(3).shuffle(ws)
    out, perm = agree(msm_pkg, sr.raw(ws), sr.CANON_LE, tag="x + k r")
    assert sr.words(out) == sorted(w % R for w in ws)
    for layout in sr.LAYOUTS:
        out, perm = agree(msm_pkg, lr.edge_records(layout) * 3, layout, tag="edge")
        assert all(w < R for w in sr.words(out))


def test_order_is_by_value_not_by_montgomery_words(msm_pkg):
    data = sr.random_column(11, 300, sr.MONT_LE)
    out, perm = agree(msm_pkg, data, sr.MONT_LE)
    by_words = sorted(range(300), key=lambda i: (sr.words(data)[i], i))
    assert perm != by_words                                   # the two orders differ on this column
    assert sr.decode(out, sr.MONT_LE) == sorted(sr.decode(data, sr.MONT_LE))


@pytest.mark.parametrize("n", [65, 4097])
def test_columns(msm_pkg, n):
    for layout in sr.LAYOUTS:
        cols = sr.random_column(1, n, layout) + sr.encode([7] * n, layout) + sr.random_column(2, n, layout)
        out, perm = agree(msm_pkg, cols, layout, n_vec=3, tag=n)
        assert perm[n:2 * n] == list(range(n)) and max(perm) == n - 1        # column-relative; all-equal: the identity


def test_forms(msm_pkg):
    layout = sr.CANON_LE
    data = sr.random_column(9, 257, layout)
    exp_out, exp_perm = sr.sort(data, layout)
    buf = ctypes.create_string_buffer(data, len(data))
    assert msm_pkg.host_fr_sort(buf, layout, n=257, out=buf, want_perm=False) == (None, None) and buf.raw == exp_out
    assert msm_pkg.host_fr_sort(b"", layout) == (b"", [])
    out = prefilled(64)
    assert msm_pkg.host_fr_sort(None, layout, n_vec=0, n=5, out=out, want_perm=False) == (None, None) and out.raw == FF * 64


def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    layout = sr.MONT_LE
    data = sr.encode([4, 1, 3, 1], layout)
    out, perm = ctypes.create_string_buffer(32 * 4), (ctypes.c_uint32 * 4)()
    big = ctypes.create_string_buffer(32 * 16)
    at = ctypes.addressof(big)
    P = ctypes.c_void_p
    good = dict(layout=layout, data=data, n=4, n_vec=1, threads=0, out=out, perm=perm)

    def call(**kw):
        x = dict(good, **kw)
        return L.msm_amd_host_fr_sort(x["layout"], x["data"], x["n"], x["n_vec"], x["threads"], x["out"], x["perm"])
    assert call() == msm_pkg.OK and list(perm) == [1, 3, 2, 0] and out.raw == sr.encode([1, 1, 3, 4], layout)
    assert call(out=None) == msm_pkg.OK and call(perm=None) == msm_pkg.OK
    errors = dict(unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), null_in=dict(data=None), no_output=dict(out=None, perm=None),
                  n_2_32=dict(n=1 << 32), product_2_32=dict(n=1 << 16, n_vec=1 << 16),
                  out_over_in=dict(data=P(at), out=P(at + 32 * 3)), out_under_in=dict(data=P(at + 32), out=P(at)),
                  perm_in_in=dict(data=P(at), perm=P(at + 32 * 3)), perm_in_out=dict(out=P(at), perm=P(at + 32 * 4 - 4)),
                  perm_over_out=dict(out=P(at + 8), perm=P(at)))
    for name, kw in errors.items():
        assert call(**kw) == msm_pkg.INPUT_ERROR, name
    assert call(data=None, n=0) == msm_pkg.OK and call(data=None, n_vec=0) == msm_pkg.OK
    assert call(n=0, out=None, perm=None) == msm_pkg.INPUT_ERROR and call(n=0, layout=99) == msm_pkg.INPUT_ERROR
    ctypes.memmove(at, data, len(data))
    assert call(data=P(at), out=P(at), perm=P(at + 32 * 4)) == msm_pkg.OK     # in place, and adjacent is disjoint
    assert ctypes.string_at(at, 32 * 4) == sr.encode([1, 1, 3, 4], layout)


@pytest.mark.parametrize("mask", MASKS)
def test_plan(msm_pkg, mask):
    for n, n_vec in ((1, 1), (4096, 1), (4097, 3), (1 << 22, 2)):
        got = msm_pkg.test_fr_sort_plan(n, n_vec, mask)
        exp = sr.plan(n, n_vec, mask)
        assert {k: got[k] for k in exp} == exp, (n, n_vec, hex(mask))
        # the record, 32 bytes of key per record, two arrays of pairs and the histograms of one column: no term has the mask
        assert got["bytes"] == 64 + 32 * n * n_vec + 16 * n + 4 * 256 * (exp["tiles"] + 1)
    out = (ctypes.c_uint64 * 4)()
    L = msm_pkg.lib()
    for bad in ((0, 1), (1, 0), (1 << 32, 1), (1 << 16, 1 << 16)):
        assert L.msm_amd_test_fr_sort_plan(bad[0], bad[1], mask, out) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_test_fr_sort_plan(1, 1, mask, None) == msm_pkg.INPUT_ERROR


def test_model_self_check_digit_masks():
    """A self-check of sort_ref.digit_mask; it calls nothing in the library: the digit masks the GPU tests expect of their
    columns, from the definition"""
    layout = sr.CANON_LE
    assert sr.digit_mask(sr.encode([7] * 9, layout), layout) == 0
    assert sr.digit_mask(sr.random_column(1, 500, layout, below=1 << 16), layout) == 0x3
    assert sr.digit_mask(sr.encode([(a << 248) + 5 for a in range(0x30)], layout), layout) == 0x80000000
    assert sr.digit_mask(sr.encode([a + (b << 136) for a in range(9) for b in range(9)], layout), layout) == 0x00020001
    assert sr.digit_mask(sr.random_column(2, 3000, layout), layout) == 0xFFFFFFFF


def test_exports(msm_pkg):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msm_amd.h")).read()
    for name in ("msm_amd_fr_sort", "msm_amd_host_fr_sort", "msm_amd_test_fr_sort_plan"):
        assert name in msm_pkg.EXPORTS and ("int %s(" % name) in header
        assert getattr(msm_pkg.lib(), name)
    assert "MSM_AMD_MEM_HOST = 0, MSM_AMD_MEM_DEVICE = 1" in header
    assert (msm_pkg.MEM_HOST, msm_pkg.MEM_DEVICE) == (sr.MEM_HOST, sr.MEM_DEVICE) == (0, 1)
