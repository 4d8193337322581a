"""The host twins of the lookup calls (msm_amd_host_fr_lookup_multiplicities, msm_amd_host_fr_prefix_sum,
msm_amd_host_fr_shift) and the pure plan tap against the big-integer model of tests/lookup_ref.py, on the CPU.  Every
comparison is of bytes.  tests/test_gpu_lookup.py pins the device calls to the twin and the model."""
import ctypes
import random

import pytest

import lookup_ref as lr

R = lr.R
ROWS = [1, 2, 63, 64, 65, 257]
INPUTS = [1, 63, 64, 65, 257, 1000]


def agree(msm_pkg, table, data, layout, n_vec=1, threads=0, tag=None):
    exp_m, exp_idx, exp_rep = lr.multiplicities(table, data, layout)
    m, idx, rep = msm_pkg.host_fr_lookup_multiplicities(table, data, msm_pkg.LOOKUP_COUNT_MISSING, layout, n_vec, threads)
    assert lr.first_difference(m, exp_m) is None, tag
    assert idx == exp_idx and rep == exp_rep, (tag, rep, exp_rep)
    total = len(data) // 32
    assert sum(lr.decode(m, layout)) == total - rep["n_missing"], tag
    if not rep["n_missing"]:
        m2, idx2, rep2 = msm_pkg.host_fr_lookup_multiplicities(table, data, msm_pkg.LOOKUP_STRICT, layout, n_vec, threads)
        assert (m2, idx2, rep2) == (m, idx, rep), tag
    return m, idx, rep


@pytest.mark.parametrize("layout", lr.LAYOUTS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_sizes(msm_pkg, n_rows, layout):
    table = lr.random_table(n_rows, n_rows, layout)
    for n in INPUTS:
        for n_vec in (1, 3):
            data = lr.draws(n + n_vec, table, layout, n * n_vec)
            agree(msm_pkg, table, data, layout, n_vec, tag=(n_rows, n, n_vec))


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_words_equal_mod_r_match(msm_pkg, layout):
    """0, r and 2^256 - 1 ... as words of a record: r is 0, r + 5 is 5, in the table and in the inputs"""
    edge = lr.edge_records(layout)
    table = edge + lr.encode([5, 7], layout)
    vals = lr.decode(table, layout)
    data = lr.encode(vals, layout) + edge + lr.raw([R + 5, 5])    # every row's value as a reduced record, then the raw words
    m, idx, rep = agree(msm_pkg, table, data, layout)
    assert rep["n_missing"] == 0
    assert idx[0] == idx[3] == 0 and lr.decode(m, layout)[3] == 0  # the row r is a duplicate of the row 0: it gets nothing
    assert idx[6] == vals.index(5) and idx[-1] == idx[-2] == 4    # CANON_LE: 5 sits at the row whose word is r + 5
    agree(msm_pkg, lr.raw([R, 0, R + 5, 5]), lr.raw([0, R, 5, R + 5, 2 * R]), layout)


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_duplicate_rows(msm_pkg, layout):
    rng = random.Random(5)
    vals = [rng.randrange(R) for _ in range(40)]
    pairs = lr.encode([v for v in vals for _ in (0, 1)], layout)
    run = lr.encode(vals[:10] + [vals[3]] * 64 + vals[10:], layout)
    same = lr.encode([vals[7]] * 130, layout)
    for table in (pairs, run, same):
        data = lr.draws(9, table, layout, 300)
        m, idx, rep = agree(msm_pkg, table, data, layout)
        reps = lr.representatives(table, layout)
        assert set(idx) <= set(reps.values())
    m, idx, rep = agree(msm_pkg, same, lr.draws(1, same, layout, 77), layout)
    assert set(idx) == {0} and rep == dict(n_missing=0, first_missing=lr.NO_MISS, rows_hit=1, max_multiplicity=77)


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_misses(msm_pkg, layout):
    table = lr.random_table(3, 65, layout, distinct=40)
    for n_vec, miss_at in ((1, (199,)), (3, (4, 100, 299)), (1, tuple(range(300)))):
        data = lr.draws(11, table, layout, 300, miss_at)
        m, idx, rep = agree(msm_pkg, table, data, layout, n_vec)
        assert rep["n_missing"] == len(miss_at) and rep["first_missing"] == miss_at[0]
        assert all(idx[i] == lr.NOT_FOUND for i in miss_at)
        buf = ctypes.create_string_buffer(b"\xFF" * (32 * 65), 32 * 65)
        with pytest.raises(msm_pkg.MsmError) as e:
            msm_pkg.host_fr_lookup_multiplicities(table, data, msm_pkg.LOOKUP_STRICT, layout, n_vec, m_out=buf)
        assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == rep and e.value.idx == idx
        assert buf.raw == b"\xFF" * (32 * 65)                     # untouched


def test_threads_and_empty(msm_pkg):
    table = lr.random_table(8, 257, lr.MONT_LE, distinct=100)
    data = lr.draws(2, table, lr.MONT_LE, 1000, (17, 900))
    got = [agree(msm_pkg, table, data, lr.MONT_LE, 1, threads) for threads in (1, 3, 16)]
    assert got[0] == got[1] == got[2]
    for n_vec, d in ((1, b""), (0, b"")):
        m, idx, rep = msm_pkg.host_fr_lookup_multiplicities(table, d, msm_pkg.LOOKUP_STRICT, lr.MONT_LE, n_vec)
        assert m == bytes(32 * 257) and idx == [] and set(rep.values()) == {0}


@pytest.mark.parametrize("n_rows", ROWS + [1 << 12, (1 << 12) + 1, (1 << 31) - 1])
def test_plan_tap(msm_pkg, n_rows):
    for bits in (32, 3, 0):
        p = msm_pkg.test_fr_lookup_plan(n_rows, bits)
        cap = p["capacity"]
        assert cap >= 2 * n_rows and cap & (cap - 1) == 0 and (cap < 4 * n_rows or cap == 2)
        assert p["home_bits"] == min(bits, cap.bit_length() - 1)
        assert p["slots_off"] == 32 * n_rows and p["bytes"] == 32 * n_rows + 4 * cap + 32
    for bad in ((0, 32), (1 << 31, 32), (5, 33)):
        with pytest.raises(msm_pkg.MsmError):
            msm_pkg.test_fr_lookup_plan(*bad)


def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    table, data = lr.encode([1, 2, 3], lr.MONT_LE), lr.encode([1, 1, 2, 3], lr.MONT_LE)
    m = ctypes.create_string_buffer(32 * 3)
    idx = (ctypes.c_uint32 * 4)()
    rep = (ctypes.c_uint64 * 4)()
    big = ctypes.create_string_buffer(32 * 8)
    at = ctypes.addressof(big)
    good = dict(layout=lr.MONT_LE, mode=0, table=table, n_rows=3, data=data, n=4, n_vec=1, threads=0, m=m, idx=idx, rep=rep)

    def call(**kw):
        a = dict(good, **kw)
        return L.msm_amd_host_fr_lookup_multiplicities(a["layout"], a["mode"], a["table"], a["n_rows"], a["data"], a["n"],
                                                       a["n_vec"], a["threads"], a["m"], a["idx"], a["rep"])
    assert call() == msm_pkg.OK and list(rep) == [0, lr.NO_MISS, 3, 2]
    assert call(idx=None) == msm_pkg.OK
    errors = dict(unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32), unknown_mode=dict(mode=2), negative_mode=dict(mode=-1),
                  null_table=dict(table=None), no_rows=dict(n_rows=0), rows_2_31=dict(n_rows=1 << 31),
                  null_in=dict(data=None), null_m=dict(m=None), null_report=dict(rep=None),
                  n_2_32=dict(n=1 << 32), product_2_32=dict(n=1 << 16, n_vec=1 << 16),
                  m_over_in=dict(data=ctypes.c_void_p(at), m=ctypes.c_void_p(at + 32 * 3)),
                  m_is_in=dict(data=ctypes.c_void_p(at), m=ctypes.c_void_p(at)),
                  idx_over_in=dict(data=ctypes.c_void_p(at), idx=ctypes.c_void_p(at + 32 * 4 - 4)),
                  idx_over_m=dict(m=ctypes.c_void_p(at), idx=ctypes.c_void_p(at + 32 * 3 - 4)))
    for name, kw in errors.items():
        assert call(**kw) == msm_pkg.INPUT_ERROR, name
    assert call(data=None, n=0) == msm_pkg.OK and call(data=None, n_vec=0) == msm_pkg.OK
    ctypes.memmove(at, data, len(data))
    assert call(data=ctypes.c_void_p(at), m=ctypes.c_void_p(at + 32 * 4)) == msm_pkg.OK      # adjacent is disjoint


# ---- running sums and the shift ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", lr.LAYOUTS)
@pytest.mark.parametrize("n", [1, 511, 512, 513])
def test_prefix_sum(msm_pkg, n, layout):
    rng = random.Random(n)
    for n_vec in (1, 3):
        vals = [rng.randrange(R) for _ in range(n * n_vec)]
        data = lr.encode(vals, layout)
        if n > 2:
            data = lr.raw([R, (1 << 256) - 1]) + data[64:]        # unreduced words are taken mod r
        for mode in (lr.INCLUSIVE, lr.EXCLUSIVE):
            exp = lr.prefix_sum(data, layout, mode, n_vec)
            for threads in (1, 3, 16):
                assert lr.first_difference(msm_pkg.host_fr_prefix_sum(data, mode, layout, n_vec, threads), exp) is None
            buf = ctypes.create_string_buffer(data, len(data))     # in place
            assert msm_pkg.lib().msm_amd_host_fr_prefix_sum(layout, mode, buf, n, n_vec, 3, buf) == msm_pkg.OK
            assert buf.raw == exp
    assert msm_pkg.host_fr_prefix_sum(b"", n_vec=1) == b""
    L = msm_pkg.lib()
    one = ctypes.create_string_buffer(64)
    assert L.msm_amd_host_fr_prefix_sum(layout, 2, one, 2, 1, 0, one) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_prefix_sum(msm_pkg.SCALAR_CANON_BE32, 0, one, 2, 1, 0, one) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_prefix_sum(layout, 0, None, 2, 1, 0, one) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_prefix_sum(layout, 0, one, 1 << 16, 1 << 16, 0, one) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_prefix_sum(layout, 0, ctypes.c_void_p(ctypes.addressof(one)), 1, 1, 0,
                                        ctypes.c_void_p(ctypes.addressof(one) + 16)) == msm_pkg.INPUT_ERROR


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_shift(msm_pkg, layout):
    rng = random.Random(7)
    for n in (1, 255, 256, 257):
        a = lr.raw(lr.EDGE_WORDS)[:32 * min(n, 6)] + lr.encode([rng.randrange(R) for _ in range(max(0, n - 6))], layout)
        for kw in (0, 1, R - 1, R, (1 << 256) - 1):
            k = lr.raw([kw])
            exp = lr.shift(a, k, layout)
            for threads in (1, 3, 16):
                assert lr.first_difference(msm_pkg.host_fr_shift(a, k, layout, threads), exp) is None, (n, kw)
            buf = ctypes.create_string_buffer(a, len(a))
            assert msm_pkg.lib().msm_amd_host_fr_shift(layout, k, buf, n, 2, buf) == msm_pkg.OK and buf.raw == exp
    L = msm_pkg.lib()
    buf, k = ctypes.create_string_buffer(64), bytes(32)
    at = ctypes.addressof(buf)
    assert L.msm_amd_host_fr_shift(layout, k, None, 0, 0, None) == msm_pkg.OK
    assert L.msm_amd_host_fr_shift(msm_pkg.SCALAR_CANON_BE32, k, buf, 2, 0, buf) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_shift(layout, None, buf, 2, 0, buf) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_shift(layout, k, None, 2, 0, buf) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_shift(layout, k, buf, 2, 0, None) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_shift(layout, k, buf, 1 << 32, 0, buf) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_fr_shift(layout, k, ctypes.c_void_p(at), 1, 0, ctypes.c_void_p(at + 16)) == msm_pkg.INPUT_ERROR
    # a seventh op of the map stays unknown: the shift is an entry point of its own
    assert L.msm_amd_host_fr_map(6, layout, k, buf, buf, buf, 2, 0, buf) == msm_pkg.INPUT_ERROR
