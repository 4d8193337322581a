"""Guard bands round every output of the host twins (msm_amd_host_*), no GPU: each twin is called through lib() with its
outputs in a tests/guard.py HostArena, because the Python wrappers allocate exactly the bytes of an output (or more:
sumcheck_round's g_out, poly_eval's y_out) and so hide its neighbourhood.  The bytes inside an output are compared with
the big-integer models (tests/guard_cases.py), the bytes round it with the seeded fill.  A twin runs the bodies the
kernels run, so a tail loop that goes one record too far or a store wider than its record shows here first.

The harness is shown to be sensitive by its own self-check below.  What it cannot see: reads past an input, writes further
away than the guard width, writes into memory the library owns."""
import ctypes
import os
import re

import pytest

import guard
import guard_cases as gc
import mle_ref
from guard import HostArena, In, Out, guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(msm_pkg):
    return msm_pkg.lib()


def call(fn, *args, ok=0):
    with HostArena() as arena:
        return guarded(arena, fn, *args, ok=ok)


# ---- the harness itself -----------------------------------------------------------------------------------------------------------
def test_harness_sees_one_byte_on_either_side():
    with HostArena() as a:
        a.add("in", data=b"\x11" * 64, readonly=True)
        out = a.add("is_one", 3)
        a.add("tail", 40)
        assert out.off % 16 == 0 and a.regions["tail"].off % 16 == 0
        a.commit().verify()
        assert a.get("in") == b"\x11" * 64 and a.image[out.end:out.end + 1] != b""
        for offset, side, text in ((out.end, "rear", "+0..+0"), (out.off - 1, "front", "-1..-1")):
            a.commit()
            a.poke(offset, bytes([a.image[offset] ^ 0x80]))
            with pytest.raises(guard.GuardError) as e:
                a.verify()
            assert "'is_one' (3 bytes) %s: offsets %s changed, 1 bytes" % (side, text) in str(e.value), e.value
            assert "'in'" not in str(e.value) and "'tail'" not in str(e.value)
            with pytest.raises(guard.GuardError):
                a.unchanged()
        a.commit()
        a.poke(a.regions["in"].off + 5, b"\x12")                       # a read-only region is held like a guard
        with pytest.raises(guard.GuardError) as e:
            a.verify()
        assert "'in' (64 bytes) read-only: offsets +5..+5" in str(e.value)
        a.commit()
        a.poke(out.off, b"\x00\xFF\x00")                               # an output may change ...
        a.verify()
        with pytest.raises(guard.GuardError):                          # ... but not under unchanged()
            a.unchanged()
        a.commit()
        a.poke(out.end, bytes(x ^ 0xFF for x in a.image[out.end:out.end + 13]))
        with pytest.raises(guard.GuardError) as e:
            a.verify()
        assert "rear: offsets +0..+12 changed, 13 bytes" in str(e.value)   # a length rounded up to 16


def test_harness_fill_is_no_constant_and_differs_per_commit():
    with HostArena() as a:
        r = a.add("out", 32, writable=[(0, 8)])
        a.commit()
        first = a.image
        assert len(set(first)) > 200 and guard.GUARD >= 4096 and a.total >= 2 * guard.GUARD + 32
        a.commit()
        assert a.image != first
        a.poke(r.off + 8, bytes([a.image[r.off + 8] ^ 1]))             # outside the writable range of a strided output
        with pytest.raises(guard.GuardError) as e:
            a.verify()
        assert "'out' (32 bytes) gap: offsets +8..+8" in str(e.value)


# ---- Fr vectors: W = kFrMapThreads = 256 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.FR_MAP_N)
def test_fr_map_shift_lincomb_inverse(L, n):
    for op in range(6):
        layout, a, b, c, k, exp = gc.fr_map_case(op, n)
        assert call(L.msm_amd_host_fr_map, op, layout, k, In(a), In(b), In(c), n, 3, Out(32 * n)) == [exp], op
        io = Out(data=a)                                               # in place: out == a
        assert call(L.msm_amd_host_fr_map, op, layout, k, io, In(b), In(c), n, 3, io) == [exp], op
    layout, a, k, exp = gc.fr_shift_case(n)
    assert call(L.msm_amd_host_fr_shift, layout, k, In(a), n, 3, Out(32 * n)) == [exp]
    io = Out(data=a)
    assert call(L.msm_amd_host_fr_shift, layout, k, io, n, 3, io) == [exp]
    layout, a, k, exp = gc.fr_lincomb_case(n)
    assert call(L.msm_amd_host_fr_lincomb, layout, k, In(a), n, gc.N_VEC, 3, Out(32 * n)) == [exp]
    layout, a, exp, zeros = gc.fr_inverse_case(n)
    nz = ctypes.c_uint64(99)
    assert call(L.msm_amd_host_fr_batch_inverse, layout, In(a), n, 3, Out(32 * n), ctypes.byref(nz)) == [exp]
    assert nz.value == zeros
    io = Out(data=a)
    assert call(L.msm_amd_host_fr_batch_inverse, layout, io, n, 3, io, None) == [exp]


# ---- scans: one tile of 2^kFrTileLog = 512 records +- 1; the sizes of the small-tile plans -------------------------------------------
@pytest.mark.parametrize("kind", ["product", "sum"])
@pytest.mark.parametrize("n", gc.FR_SCAN_N + gc.FR_SCAN_SMALL_TILE_N)
def test_fr_prefix_scans(L, kind, n):
    fn = L.msm_amd_host_fr_prefix_product if kind == "product" else L.msm_amd_host_fr_prefix_sum
    for mode in (0, 1):
        layout, a, exp = gc.fr_scan_case(kind, n, mode)
        assert call(fn, layout, mode, In(a), n, gc.N_VEC, 3, Out(len(a))) == [exp], mode
        io = Out(data=a)
        assert call(fn, layout, mode, io, n, gc.N_VEC, 3, io) == [exp], mode


@pytest.mark.parametrize("n", gc.FR_SCAN_N)
def test_fr_poly_eval_and_div_linear(L, n):
    """y_out and rem_out are n_vec records (the wrappers pass exactly that many, but never look behind them)"""
    layout, a, z, y, q, rem = gc.fr_poly_case(n)
    assert call(L.msm_amd_host_fr_poly_eval, layout, z, In(a), n, gc.N_VEC, 3, Out(32 * gc.N_VEC)) == [y]
    assert call(L.msm_amd_host_fr_poly_div_linear, layout, z, In(a), n, gc.N_VEC, 3, Out(len(a)), Out(32 * gc.N_VEC)) == [q, rem]
    assert call(L.msm_amd_host_fr_poly_div_linear, layout, z, In(a), n, gc.N_VEC, 3, Out(len(a)), None) == [q]
    io = Out(data=a)
    assert call(L.msm_amd_host_fr_poly_div_linear, layout, z, io, n, gc.N_VEC, 3, io, Out(32 * gc.N_VEC)) == [q, rem]


# ---- sparse product: rows round one wave (64) and one workgroup (256) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", gc.MATVEC_ROWS)
def test_fr_matvec(msm_pkg, L, n_rows):
    layout, mat, x, exp = gc.matvec_case(n_rows)
    rows, cols, row_ptr, col_idx, values = mat.c_args()
    args = (layout, rows, cols, msm_pkg._csr_u64(row_ptr), msm_pkg._csr_u32(col_idx), values)
    assert call(L.msm_amd_host_fr_matvec, *args, In(x), 3, Out(32 * n_rows)) == [exp]


# ---- multilinear tables: n = 2 .. 1024, both orders, stride = n and stride = n + 3 ---------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "stride_n_plus_3"])
@pytest.mark.parametrize("n", gc.MLE_N)
def test_fr_mle_bind(L, n, strided):
    m = n.bit_length() - 1
    for order in mle_ref.ORDERS:
        for n_bind in sorted({1, min(2, m), m}):
            layout, stride, data, r, exp = gc.mle_bind_case(n, order, n_bind, strided)
            span = 32 * ((gc.N_VEC - 1) * stride + n // 2)
            out = Out(span, writable=gc.mle_bind_writable(n, stride))
            got, = call(L.msm_amd_host_fr_mle_bind, layout, order, r, n_bind, In(data), n, gc.N_VEC, stride, 3, out)
            assert mle_ref.bind_outputs(got, n, n_bind, gc.N_VEC, stride) == exp, (order, n_bind)
    layout, stride, data, r, exp = gc.mle_bind_case(n, mle_ref.HIGH, 1, strided)      # in place is HIGH's alone
    io = Out(data=data, writable=gc.mle_bind_writable(n, stride))
    got, = call(L.msm_amd_host_fr_mle_bind, layout, mle_ref.HIGH, r, 1, io, n, gc.N_VEC, stride, 3, io)
    assert mle_ref.bind_outputs(got, n, 1, gc.N_VEC, stride) == exp


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "stride_n_plus_3"])
@pytest.mark.parametrize("n", gc.MLE_N)
def test_fr_mle_eval_eq_table_and_sumcheck_round(msm_pkg, L, n, strided):
    m = n.bit_length() - 1
    for order in mle_ref.ORDERS:
        layout, stride, data, point, exp = gc.mle_eval_case(n, order, strided)
        assert call(L.msm_amd_host_fr_mle_eval, layout, order, point, In(data), n, gc.N_VEC, stride, 3, Out(32 * gc.N_VEC)) == [exp]
        if not strided:
            layout, point, exp = gc.mle_eq_case(m, order)
            assert call(L.msm_amd_host_fr_eq_table, layout, order, point, m, 3, Out(32 * n)) == [exp]
        for form, n_vec in gc.MLE_ROUND_SHAPES:
            layout, stride, data, exp = gc.mle_round_case(n, order, form, n_vec, strided)
            values = msm_pkg.sumcheck_values(form, n_vec)              # d + 1 records, not the 5 the wrapper passes
            assert len(exp) == 32 * values
            got = call(L.msm_amd_host_fr_sumcheck_round, layout, order, form, In(data), n, n_vec, stride, 3, Out(32 * values))
            assert got == [exp], (order, form, n_vec)


# ---- Poseidon: n states or messages round one wave (64) and one workgroup (256), every t ----------------------------------------------------------------------
@pytest.mark.parametrize("t", gc.POSEIDON_T)
def test_poseidon_permute_and_hash(L, t):
    import poseidon_ref as ps
    for n in gc.POSEIDON_N:
        layout, data, exp = gc.poseidon_permute_case(t, n)
        _, _, ark, mds = gc.poseidon_constants(t, layout)
        shape = (t, ps.R_F, ps.R_P[t], layout, ark, mds)
        assert call(L.msm_amd_host_poseidon_permute, *shape, In(data), n, 3, Out(len(data))) == [exp], n
        io = Out(data=data)
        assert call(L.msm_amd_host_poseidon_permute, *shape, io, n, 3, io) == [exp], n
        layout, data, tag, exp = gc.poseidon_hash_case(t, n)
        _, _, ark, mds = gc.poseidon_constants(t, layout)
        shape = (t, ps.R_F, ps.R_P[t], layout, ark, mds)
        assert call(L.msm_amd_host_poseidon_hash, *shape, tag, In(data), n, 3, Out(32 * n)) == [exp], n
        if t == 2:                                                     # "out == in is allowed for t = 2 only"
            io = Out(data=data)
            assert call(L.msm_amd_host_poseidon_hash, *shape, tag, io, n, 3, io) == [exp], n


@pytest.mark.parametrize("t,n_leaves", gc.MERKLE_SHAPES)
def test_poseidon_merkle_build_and_paths(msm_pkg, L, t, n_leaves):
    import poseidon_ref as ps
    layout, leaves, tag, tree, root, idx, paths = gc.merkle_case(t, n_leaves)
    _, _, ark, mds = gc.poseidon_constants(t, layout)
    shape = (t, ps.R_F, ps.R_P[t], layout, ark, mds)
    build = L.msm_amd_host_poseidon_merkle_build
    assert call(build, *shape, tag, In(leaves), n_leaves, 3, Out(len(tree)), Out(32)) == [tree, root]     # root32: 32 bytes
    assert call(build, *shape, tag, In(leaves), n_leaves, 3, Out(len(tree)), None) == [tree]
    ids = msm_pkg._csr_u64(idx)
    got = call(L.msm_amd_host_poseidon_merkle_paths, t, layout, In(leaves), n_leaves, In(tree), ids, len(idx), 3, Out(len(paths)))
    assert got == [paths]


def test_poseidon_merkle_refuses_a_leaf_count_that_is_no_power_of_the_arity(msm_pkg, L):
    """include/msm_amd.h: "n_leaves = a^d leaves, d >= 1; any other count is MSM_AMD_INPUT_ERROR": nothing is written"""
    import poseidon_ref as ps
    t, n_leaves = gc.MERKLE_BAD_LEAVES
    _, _, ark, mds = gc.poseidon_constants(t, gc.MONT_LE)
    with HostArena() as a:
        leaves, tree, root = a.add("leaves", 32 * n_leaves), a.add("tree", 32 * n_leaves), a.add("root", 32)
        a.commit()
        p = ctypes.c_void_p
        st = L.msm_amd_host_poseidon_merkle_build(t, ps.R_F, ps.R_P[t], gc.MONT_LE, ark, mds, None, p(leaves.ptr), n_leaves, 3,
                                                  p(tree.ptr), p(root.ptr))
        assert st == msm_pkg.INPUT_ERROR
        a.unchanged()


# ---- lookups: n_rows round 64 and kLookupThreads = 256; totals round kLookupThreads = 256 and kLookupBlockThreads = 1024 ---------------------------------
@pytest.mark.parametrize("n_rows", gc.LOOKUP_ROWS)
def test_fr_lookup_multiplicities(msm_pkg, L, n_rows):
    import struct
    fn = L.msm_amd_host_fr_lookup_multiplicities
    for total in gc.LOOKUP_TOTAL:
        layout, table, data, n_vec, m, idx, rep = gc.lookup_case(n_rows, total)
        want_idx = struct.pack("<%dI" % total, *idx)                     # 4 total bytes: no multiple of 16 for an odd total
        report = (ctypes.c_uint64 * 4)()
        args = (layout, msm_pkg.LOOKUP_COUNT_MISSING, In(table), n_rows, In(data), total // n_vec, n_vec, 3)
        assert call(fn, *args, Out(32 * n_rows), Out(4 * total), report) == [m, want_idx], total
        assert dict(zip(msm_pkg.LOOKUP_REPORT_FIELDS, report)) == rep
        assert call(fn, *args, Out(32 * n_rows), None, report) == [m], total
    layout, table, data, n_vec, m, idx, rep = gc.lookup_case(n_rows, 257, miss=True)
    with HostArena() as a:                                             # a STRICT miss: m_out and its guards unchanged
        d_t, d_in, d_m = a.add("table", data=table, readonly=True), a.add("in", data=data, readonly=True), a.add("m", 32 * n_rows)
        a.commit()
        p, report = ctypes.c_void_p, (ctypes.c_uint64 * 4)()
        assert fn(layout, msm_pkg.LOOKUP_STRICT, p(d_t.ptr), n_rows, p(d_in.ptr), 257, 1, 3, p(d_m.ptr), None, report) == msm_pkg.INPUT_ERROR
        assert report[0] == 1 and report[1] == 256
        a.unchanged()


# ---- points: n = 1, 3, 63, 65, and 255 .. 257 where a kernel launches 256 threads -------------------------------------------------------------------------
import check_ref as c                          # noqa: E402
import compress_ref as cr                      # noqa: E402
import mul_ref as mr                           # noqa: E402
import ntt_ref                                 # noqa: E402
import pairing_ref as pr                       # noqa: E402


@pytest.mark.parametrize("group", [1, 2])
def test_check_points_reasons_are_n_bytes(msm_pkg, L, group):
    """reasons is n BYTES: its rear guard is not dword aligned"""
    fn = L.msm_amd_host_check_points if group == 1 else L.msm_amd_host_g2_check_points
    for n in gc.check_sizes(group):
        layout, checks, data, reasons, report = gc.check_case(group, n)
        rep = msm_pkg.CheckReport()
        assert call(fn, layout, In(data), n, checks, 3, Out(n), ctypes.byref(rep)) == [reasons], n
        assert c.same_report(rep.as_dict(), report)
        assert call(fn, layout, In(data), n, checks, 3, None, ctypes.byref(rep)) == []
        assert c.same_report(rep.as_dict(), report)


@pytest.mark.parametrize("group", [1, 2])
def test_decompress_and_compress_points(msm_pkg, L, group):
    dec = L.msm_amd_host_decompress_points if group == 1 else L.msm_amd_host_g2_decompress_points
    com = L.msm_amd_host_compress_points if group == 1 else L.msm_amd_host_g2_compress_points
    for n in gc.COMPRESS_N:
        for fmt in gc.FORMATS:
            data, _, reasons, report, outs = gc.decompress_case(group, n, fmt)
            for lo, want in outs.items():
                rep = msm_pkg.DecompressReport()
                assert call(dec, fmt, In(data), n, lo, 3, Out(len(want)), Out(n), ctypes.byref(rep)) == [want, reasons], (n, fmt, lo)
                assert cr.same_report(rep.as_dict(), report)
                assert call(dec, fmt, In(data), n, lo, 3, Out(len(want)), None, ctypes.byref(rep)) == [want]
                pts, want_c, n_bad = gc.compress_case(group, n, fmt, lo)
                bad = ctypes.c_uint64(77)
                assert call(com, lo, In(pts), n, fmt, 3, Out(len(want_c)), ctypes.byref(bad)) == [want_c], (n, fmt, lo)
                assert bad.value == n_bad


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("mode", [mr.EACH, mr.ONE])
def test_mul_points(L, group, mode):
    fn = L.msm_amd_host_mul_points if group == 1 else L.msm_amd_host_g2_mul_points
    for n in gc.mul_sizes(group):
        sl, li, scalars, pts, want = gc.mul_case(group, n, mode)
        for lo in gc.mul_out_layouts(group, n):
            exp = gc.point_records(group, lo, want)
            assert call(fn, sl, li, mode, In(scalars), In(pts), n, lo, 3, Out(len(exp))) == [exp], (n, lo)


@pytest.mark.parametrize("n_groups,group_size", gc.PAIRING_SHAPES)
def test_pairing_product_and_final_exponentiation(L, n_groups, group_size):
    """is_one is n_groups BYTES; a MILLER_ONLY record is a representative: only its final exponentiation is specified"""
    l1, l2, a, b, want, one = gc.pairing_case(n_groups, group_size)
    fn, fe = L.msm_amd_host_pairing_product, L.msm_amd_host_final_exponentiation
    for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
        exp = gc.gt_records(want, gt)
        args = (l1, l2, In(a), In(b), n_groups, group_size)
        assert call(fn, *args, 0, gt, Out(len(exp)), Out(n_groups), 3) == [exp, one], gt
        assert call(fn, *args, 0, gt, Out(len(exp)), None, 3) == [exp], gt
        mil, = call(fn, *args, pr.PAIRING_MILLER_ONLY, gt, Out(len(exp)), None, 3)
        assert call(fe, gt, In(mil), n_groups, Out(len(exp)), Out(n_groups), 3) == [exp, one], gt
        io = Out(data=mil)
        assert call(fe, gt, io, n_groups, io, None, 3) == [exp], gt


# ---- transforms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(0, 11))
def test_ntt(L, log_n):
    for n_vec in (1, 3):
        for direction in ntt_ref.DIRECTIONS:
            for shifted in (False, True):
                layout, root, data, shift, exp = gc.ntt_case(log_n, n_vec, direction, shifted)
                assert call(L.msm_amd_host_ntt, root, log_n, direction, layout, shift, In(data), Out(len(data)), n_vec, 3) == [exp]
                io = Out(data=data)
                assert call(L.msm_amd_host_ntt, root, log_n, direction, layout, shift, io, io, n_vec, 3) == [exp]


@pytest.mark.parametrize("log_n", gc.NTT_POINTS_LOGS)
def test_ntt_points(L, log_n):
    for direction in ntt_ref.DIRECTIONS:
        li, root, data, want = gc.ntt_points_case(log_n, direction)
        for lo in gc.G1_OUT:
            exp = gc.point_records(1, lo, want)
            assert call(L.msm_amd_host_ntt_points, root, log_n, direction, li, In(data), lo, Out(len(exp)), 3) == [exp], (direction, lo)


# ---- MSM: the 96-byte (G1) and 192-byte (G2) result ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.MSM_N)
def test_msm_results(L, n):
    sl, scalars, pts, want = gc.msm_case(1, n)
    out, = call(L.msm_amd_host_msm, sl, 0, In(scalars), In(pts), n, 3, Out(96))
    assert gc.msm_result(1, out) == want
    sl, scalars, pts, want = gc.msm_case(1, n, bits=20)
    out, = call(L.msm_amd_host_msm_bounded, sl, 0, In(scalars), In(pts), n, 20, 0, 3, Out(96))
    assert gc.msm_result(1, out) == want
    sl, scalars, pts, want = gc.msm_case(2, n)
    out, = call(L.msm_amd_host_msm_g2, sl, 0, In(scalars), In(pts), n, 3, Out(192))
    assert gc.msm_result(2, out) == want


# ---- refused calls write nothing ---------------------------------------------------------------------------------------------------------
def test_refused_twin_calls_leave_the_whole_arena_unchanged(msm_pkg, L):
    from guard import At
    bad, n = msm_pkg.INPUT_ERROR, 65
    layout, a, k, _ = gc.fr_shift_case(n)
    io = Out(data=a)
    call(L.msm_amd_host_fr_shift, layout, k, io, n - 1, 3, At(io, 32), ok=bad)                    # partial overlap
    call(L.msm_amd_host_fr_map, 6, layout, k, In(a), In(a), In(a), n, 3, Out(32 * n), ok=bad)     # no seventh op
    call(L.msm_amd_host_fr_poly_eval, 2, k, In(a), n, 1, 3, Out(32), ok=bad)                      # CANON_BE32 is refused
    lay, stride, data, r, _ = gc.mle_bind_case(64, mle_ref.LOW, 1, False)
    io = Out(data=data)
    call(L.msm_amd_host_fr_mle_bind, lay, mle_ref.LOW, r, 1, io, 64, gc.N_VEC, stride, 3, io, ok=bad)   # LOW in place
    layout, checks, data, _, _ = gc.check_case(1, 63)
    call(L.msm_amd_host_check_points, 9, In(data), 63, checks, 3, Out(63), ctypes.byref(msm_pkg.CheckReport()), ok=bad)
    l1, l2, a1, b2, _, _ = gc.pairing_case(3, 1)
    call(L.msm_amd_host_pairing_product, l1, l2, In(a1), In(b2), 3, 1, pr.PAIRING_MILLER_ONLY, 0, Out(3 * 384), Out(3), 3, ok=bad)
    call(L.msm_amd_host_final_exponentiation, 2, In(bytes(384)), 1, Out(384), Out(1), 3, ok=bad)


# ---- every _device call of the header has a guard test, or a reason why not ----------------------------------------------------------------
def test_every_device_call_of_the_header_is_covered_or_excluded():
    header = open(os.path.join(ROOT, "include", "msm_amd.h")).read()
    declared = set(re.findall(r"\bmsm_amd_(\w+_device)\s*\(", header))
    covered, excluded = set(gc.DEVICE_CALLS_COVERED), set(gc.DEVICE_CALLS_EXCLUDED)
    assert not covered & excluded
    assert declared - covered - excluded == set(), "new _device calls without a guard-band test"
    assert (covered | excluded) - declared == set(), "names that are not in the header any more"
    assert all(reason for reason in gc.DEVICE_CALLS_EXCLUDED.values())
    gpu_file = open(os.path.join(ROOT, "tests", "test_gpu_guard_bands.py")).read()
    missing = [name for name in sorted(covered) if not re.search(r"\bL\.msm_amd_%s\b" % name, gpu_file)]
    assert not missing, missing                                       # "covered" means: called in the GPU file
    for name in excluded:
        assert "msm_amd_" + name in gpu_file.split('"""')[1], name    # and the docstring there says why not
