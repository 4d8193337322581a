"""The host twin of the sparse product (msm_amd_host_fr_matvec) against the big-integer model of tests/matvec_ref.py, its
argument checks, and the planner of the device side (msm_amd_test_fr_matrix_plan, pure host code).  No GPU.  Every
comparison is of bytes: the records of a result are unique."""
import ctypes
import os
import random
import re

import pytest

import matvec_ref as m

R = m.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msm_amd_fr_matrix_build", "msm_amd_fr_matrix_info", "msm_amd_fr_matrix_free", "msm_amd_fr_matvec",
       "msm_amd_fr_matvec_device", "msm_amd_host_fr_matvec", "msm_amd_test_fr_matrix_plan")


def twin(msm_pkg, mat, x, layout, threads=0):
    return msm_pkg.host_fr_matvec(*mat.c_args(), x, layout, threads)


def check(msm_pkg, mat, x, layout, tag):
    exp = m.matvec(mat, x, layout, layout)
    for threads in (1, 16):
        assert m.first_difference(twin(msm_pkg, mat, x, layout, threads), exp) is None, (tag, threads)


# ---- 1. symbols ---------------------------------------------------------------------------------------------------------------
def test_symbols_constants_and_exports(msm_pkg):
    L = msm_pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "msm_amd.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in msm_pkg.EXPORTS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "typedef struct msm_amd_fr_matrix msm_amd_fr_matrix;" in hdr
    assert "MSM_AMD_FR_MAT_LONG" in hdr and "MSM_AMD_FR_MAT_SEG_LOG" in hdr
    for name in ("fr_matrix_build", "fr_matrix_info", "fr_matrix_free", "fr_matvec", "fr_matvec_device"):
        assert hasattr(msm_pkg.MsmConfig, name), name
    assert callable(msm_pkg.host_fr_matvec) and callable(msm_pkg.test_fr_matrix_plan)


# ---- 2. the twin against the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_every_row_count(msm_pkg, layout):
    """every n_rows <= 70, row lengths 0 .. 9; the column count moves against the row count"""
    for n_rows in range(1, 71):
        rng = random.Random(100 + n_rows)
        n_cols = 1 + (n_rows * 7) % 23
        mat = m.from_lengths(n_rows, [rng.randrange(10) for _ in range(n_rows)], n_cols, layout)
        check(msm_pkg, mat, m.encode(m.random_values(n_rows, n_cols), layout), layout, n_rows)


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_shapes_at_the_edges(msm_pkg, layout):
    x1 = m.encode([R - 2], layout)
    # one column: every entry repeats column 0
    check(msm_pkg, m.from_lengths(1, [3, 0, 9, 1], 1, layout), x1, layout, "one column")
    x = m.encode(m.random_values(2, 5), layout)
    # all rows empty; with and without the arrays of an empty matrix
    empty = m.from_lengths(2, [0] * 7, 5, layout)
    check(msm_pkg, empty, x, layout, "all empty")
    assert msm_pkg.host_fr_matvec(7, 5, empty.row_ptr, None, None, x, layout) == bytes(32 * 7)
    check(msm_pkg, m.from_lengths(3, [0, 4, 2, 0], 5, layout), x, layout, "first and last row empty")
    check(msm_pkg, m.from_lengths(4, [0, 0, 0, 6], 5, layout), x, layout, "only the last row")
    check(msm_pkg, m.from_lengths(5, [6, 0, 0, 0], 5, layout), x, layout, "only the first row")


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_edge_words_in_values_and_x(msm_pkg, layout):
    """0, 1, r - 1, the raw words r, r + 1 and 2^256 - 1, and a random value: every pair of them meets in a product"""
    recs = m.edge_records(layout)
    k = len(recs)
    # row i holds value i against every x word; one more row holds every value against x word 0 (a sum of all)
    row_ptr = [k * i for i in range(k + 1)] + [k * k + k]
    cols = [j for _ in range(k) for j in range(k)] + [0] * k
    vals = b"".join(recs[i] for i in range(k) for _ in range(k)) + b"".join(recs)
    mat = m.Csr(k + 1, k, row_ptr, cols, vals)
    check(msm_pkg, mat, b"".join(recs), layout, "edge words")


def test_threads_do_not_show(msm_pkg):
    """ranges of equal entry count: one heavy row beside many light ones, and more threads than rows"""
    lengths = [1] * 40 + [700] + [0] * 30 + [2] * 40
    mat = m.from_lengths(9, lengths, 50, m.MONT_LE)
    x = m.encode(m.random_values(10, 50), m.MONT_LE)
    exp = m.matvec(mat, x, m.MONT_LE, m.MONT_LE)
    for threads in (1, 2, 3, 16, 64, 200):
        assert twin(msm_pkg, mat, x, m.MONT_LE, threads) == exp, threads
    small = m.from_lengths(11, [3, 2], 4, m.CANON_LE)
    xs = m.encode(m.random_values(12, 4), m.CANON_LE)
    assert twin(msm_pkg, small, xs, m.CANON_LE, 16) == m.matvec(small, xs, m.CANON_LE, m.CANON_LE)


# ---- 3. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    mat = m.from_lengths(1, [2, 0, 3], 4, m.MONT_LE)
    x = m.encode([1, 2, 3, 4], m.MONT_LE)
    ok = lambda **kw: dict(dict(n_rows=3, n_cols=4, row_ptr=mat.row_ptr, col_idx=mat.col_idx, values=mat.values, x=x,
                                scalar_layout=m.MONT_LE), **kw)   # noqa: E731
    assert msm_pkg.host_fr_matvec(**ok()) == m.matvec(mat, x, m.MONT_LE, m.MONT_LE)

    def refused(**kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            msm_pkg.host_fr_matvec(**ok(**kw))
        assert e.value.status == msm_pkg.INPUT_ERROR, kw.keys()

    refused(scalar_layout=msm_pkg.SCALAR_CANON_BE32)
    refused(scalar_layout=7)
    refused(n_rows=0, row_ptr=[0])
    refused(n_cols=0)
    refused(n_rows=1 << 32, y=ctypes.create_string_buffer(32))   # refused before row_ptr is read
    refused(n_cols=1 << 32)
    refused(row_ptr=None)
    refused(col_idx=None)
    refused(values=None)
    refused(x=None)
    refused(row_ptr=[1, 2, 2, 5])                              # row_ptr[0] = 1
    refused(row_ptr=[0, 2, 1, 5])                              # decreasing
    refused(row_ptr=[0, 2, 2, 1 << 32])                        # nnz >= 2^32 (refused before any entry is read)
    refused(col_idx=[0, 1, 2, 4, 3])                           # a column equal to n_cols
    refused(col_idx=[0, 1, 2, 3, 0xFFFFFFFF])
    # y overlapping x by one record, from either side; a null y
    buf = ctypes.create_string_buffer(32 * 8)
    ctypes.memmove(buf, x, len(x))
    base = ctypes.addressof(buf)
    L = msm_pkg.lib()
    rp = (ctypes.c_uint64 * 4)(*mat.row_ptr)
    ci = (ctypes.c_uint32 * 5)(*mat.col_idx)

    def call(x_at, y_at):
        return L.msm_amd_host_fr_matvec(m.MONT_LE, 3, 4, rp, ci, mat.values, ctypes.c_void_p(x_at), 1,
                                        ctypes.c_void_p(y_at) if y_at else None)

    assert call(base, base + 32 * 3) == msm_pkg.INPUT_ERROR    # y's first record is x's last
    assert call(base + 32 * 2, base) == msm_pkg.INPUT_ERROR    # y's last record is x's first
    assert call(base, base) == msm_pkg.INPUT_ERROR             # in place
    assert call(base, 0) == msm_pkg.INPUT_ERROR
    assert buf.raw[:len(x)] == x
    assert call(base, base + 32 * 4) == msm_pkg.OK             # touching, not overlapping
    assert buf.raw[32 * 4:32 * 7] == m.matvec(mat, x, m.MONT_LE, m.MONT_LE)


# ---- 4. the planner -----------------------------------------------------------------------------------------------------------
def plan_lengths(seed, n_rows=300):
    rng = random.Random(seed)
    pool = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, 256, 257, 700]
    return [pool[rng.randrange(len(pool))] if rng.random() < 0.3 else rng.randrange(6) for _ in range(n_rows)]


def row_ptr_of(lengths):
    out = [0]
    for ln in lengths:
        out.append(out[-1] + ln)
    return out


def check_plan(msm_pkg, lengths, long_rows, seg_log):
    """the classes partition the rows; the segments tile every wave row in order, none empty, none above SEG; partial
    slots are distinct and dense; launches and waves follow"""
    row_ptr = row_ptr_of(lengths)
    seg = 1 << seg_log
    p = msm_pkg.test_fr_matrix_plan(row_ptr, long_rows, seg_log, segs_cap=row_ptr[-1] + 1)
    wave_rows = [i for i, ln in enumerate(lengths) if ln > long_rows]
    assert p["lane_rows"] == len(lengths) - len(wave_rows) and p["wave_rows"] == len(wave_rows)
    assert len(p["segs"]) == p["segments"]
    by_row = {}
    for row, first, count, slot in p["segs"]:
        assert 1 <= count <= seg
        by_row.setdefault(row, []).append((first, count, slot))
    assert sorted(by_row) == wave_rows                          # every wave row, no lane row
    assert [s[0] for s in p["segs"]] == sorted(s[0] for s in p["segs"])   # in row order
    slots = []
    for row in wave_rows:
        at = row_ptr[row]
        for first, count, slot in by_row[row]:
            assert first == at
            at += count
            assert (slot is None) == (len(by_row[row]) == 1)
            if slot is not None:
                slots.append(slot)
        assert at == row_ptr[row + 1]
        assert all(c == seg for _, c, _ in by_row[row][:-1])    # only the last segment of a row is short
    split = [r for r in wave_rows if len(by_row[r]) > 1]
    assert slots == list(range(len(slots))) and p["partials"] == len(slots) and p["split_rows"] == len(split)
    assert p["launches"] == (3 if split else 2 if wave_rows else 1)
    assert p["waves"] == (len(lengths) + 63) // 64 + p["segments"] + p["split_rows"]
    return p


@pytest.mark.parametrize("long_rows", [1, 4, 64])
@pytest.mark.parametrize("seg_log", [6, 8])
def test_planner(msm_pkg, long_rows, seg_log):
    for seed in range(6):
        check_plan(msm_pkg, plan_lengths(seed), long_rows, seg_log)
    assert check_plan(msm_pkg, [0, 1, 1, 0], long_rows, seg_log)["launches"] == 1
    # a full segment is one wave's row -- unless LONG lets it stay on the lane path (LONG = SEG = 64)
    assert check_plan(msm_pkg, [0, 1 << seg_log, 1], long_rows, seg_log)["launches"] == (2 if long_rows < 1 << seg_log else 1)
    assert check_plan(msm_pkg, [(1 << seg_log) + 1], long_rows, seg_log)["launches"] == 3
    assert check_plan(msm_pkg, [long_rows, long_rows + 1], long_rows, seg_log)["wave_rows"] == 1
    # segs_cap cuts the list, not the counts
    p = msm_pkg.test_fr_matrix_plan(row_ptr_of([700, 700]), long_rows, seg_log, segs_cap=2)
    assert len(p["segs"]) == 2 and p["segments"] == 2 * ((700 + (1 << seg_log) - 1) >> seg_log)


def test_planner_refuses(msm_pkg):
    for bad in (dict(long_rows=0), dict(long_rows=4097), dict(seg_log=5), dict(seg_log=21)):
        with pytest.raises(msm_pkg.MsmError):
            msm_pkg.test_fr_matrix_plan([0, 3], **bad)
    for row_ptr in ([1, 3], [0, 3, 2], [0]):
        with pytest.raises(msm_pkg.MsmError):
            msm_pkg.test_fr_matrix_plan(row_ptr)


@pytest.mark.parametrize("long_rows,seg_log", [(8, 8), (32, 10), (128, 14)])
def test_load_balance_on_the_r1cs_shape(msm_pkg, long_rows, seg_log):
    """The benchmark's r1cs shape at 2^16 rows.  The lane path dispatches one wave per 64 consecutive rows and none of
    its rows is above LONG; the wave path dispatches one wave per segment and none covers more than SEG entries; the
    fold one wave per split row.  Segments <= sum over wave rows of ceil(len / SEG) <= nnz / SEG + wave rows, and split rows
    <= wave rows, so the dispatched waves stay below 2 (ceil(n_rows / 64) + ceil(nnz / SEG) + wave rows)."""
    n = 1 << 16
    mat = m.r1cs_shape(3, n)
    row_ptr = [int(v) for v in mat.row_ptr]
    lengths = [b - a for a, b in zip(row_ptr, row_ptr[1:])]
    assert max(lengths) == n // 4 and sum(1 for ln in lengths if ln == 1000) >= n // 1000
    p = check_plan(msm_pkg, lengths, long_rows, seg_log)
    seg = 1 << seg_log
    assert max(count for _, _, count, _ in p["segs"]) <= seg
    wave = {row for row, _, _, _ in p["segs"]}
    assert all(ln <= long_rows for i, ln in enumerate(lengths) if i not in wave)
    assert p["waves"] <= 2 * ((n + 63) // 64 + (mat.nnz + seg - 1) // seg + p["wave_rows"])
