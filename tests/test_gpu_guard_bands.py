"""Guard bands round every device buffer a `_device` call writes, and round the host buffers the ctx calls copy back into.

Inputs, outputs and side outputs of one call lie in one tests/guard.py Arena (device memory) -- the host outputs of a
device call (y_out, rem_out, g_out, root32, the 96 / 192-byte MSM result) in a HostArena --, the whole arena is filled from
a seeded byte stream, the call runs through lib(), the output bytes are compared with the big-integer models
(tests/guard_cases.py, the cases tests/test_guard_bands_host.py runs through the host twins) and verify() holds every byte
round the outputs, and every byte of the inputs of an out-of-place call, to the fill.  hipMalloc pads allocations and the
neighbour of an output is usually another array of the caller, so an overrun faults nowhere and shows as a wrong proof
later; GPU sanitizers are not available, which leaves this instrument.  The shapes and the unit W each straddles are listed
in guard_cases.py; the guard width in guard.py.

That the harness itself sees a stray byte is shown by test_harness_sees_one_byte_on_either_side, which writes one with
copy_to_device just behind and just in front of a 3-byte output.

What this cannot see: a read past the end of an input; a write that lands further away than the guard width; a write into
memory the library owns (the workspaces of a ctx).  PREPARED records have no model of their own: their content is read
through the multiplication call ([1] P, PREPARED in, affine out), their neighbourhood like any other.

Calls of include/msm_amd.h with `_device(` in their name that have no test here, and why (guard_cases.DEVICE_CALLS_EXCLUDED;
tests/test_guard_bands_host.py holds the two lists against the header):
  msm_amd_submit_batch_device, msm_amd_submit_batch_bounded_device, msm_amd_submit_batch_multi_device: the asynchronous
      twins of msm_amd_msm_batch_device, the same kernels on the same buffers
  msm_amd_msm_batch_bounded_device, msm_amd_msm_batch_multi_device: msm_amd_msm_batch_device at a width / over several
      ctxs; the bounded plan is covered by msm_amd_msm_bounded_device
  msm_amd_tables_build_device, msm_amd_g2_tables_build_device: they write only memory the library allocates itself
  msm_amd_copy_to_device, msm_amd_ctx_device, msm_amd_pin_thread_to_device: no compute calls (the first is the harness's
      own upload)"""
import ctypes
import struct

import pytest

import check_ref as c
import compress_ref as cr
import guard
import guard_cases as gc
import mle_ref
import mul_ref as mr
import ntt_ref
import ntt_shapes
import pairing_ref as pr
from guard import Arena, At, HostArena, In, Out, guarded

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def L(msm_pkg):
    return msm_pkg.lib()


def call(cfg, fn, *args, ok=0):
    """fn(ctx, ...) with the device buffers in an Arena of cfg and the host=True ones in a HostArena"""
    with Arena(cfg) as arena, HostArena() as host:
        return guarded(arena, fn, cfg.h, *args, ok=ok, host_arena=host)


def host_call(cfg, fn, *args, ok=0):
    """a host-buffer form: every buffer in one HostArena"""
    with HostArena() as host:
        return guarded(host, fn, cfg.h, *args, ok=ok)


def HOut(nbytes):
    return Out(nbytes, host=True)


@pytest.fixture
def tiles_of_four(msm_pkg, monkeypatch):
    monkeypatch.setenv("MSM_AMD_FR_TILE_LOG", "2")
    c2 = msm_pkg.setup_metal_state()
    yield c2
    c2.close()


# ---- the harness itself: one byte behind an output, one byte in front of it -----------------------------------------------------
def test_harness_sees_one_byte_on_either_side(cfg):
    with Arena(cfg) as a:
        a.add("in", data=b"\x11" * 64, readonly=True)
        out = a.add("is_one", 3)
        a.add("tail", 40)
        a.commit().verify()
        assert a.get("in") == b"\x11" * 64
        for offset, side, text in ((out.end, "rear", "+0..+0"), (out.off - 1, "front", "-1..-1")):
            a.commit()
            cfg.to_device(a.base + offset, bytes([a.image[offset] ^ 0x80]))
            with pytest.raises(guard.GuardError) as e:
                a.verify()
            assert "'is_one' (3 bytes) %s: offsets %s changed, 1 bytes" % (side, text) in str(e.value), e.value
            assert "'in'" not in str(e.value) and "'tail'" not in str(e.value)
            with pytest.raises(guard.GuardError):
                a.unchanged()
        a.commit()
        cfg.to_device(out.ptr, bytes(x ^ 0xFF for x in a.image[out.off:out.end]))     # the output itself may change
        a.verify()
        with pytest.raises(guard.GuardError):
            a.unchanged()


# ---- Fr vectors: W = kFrMapThreads = 256 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gc.FR_MAP_N)
def test_fr_map_shift_lincomb_inverse(cfg, L, n):
    for op in range(6):
        layout, a, b, cc, k, exp = gc.fr_map_case(op, n)
        assert call(cfg, L.msm_amd_fr_map_device, op, layout, k, In(a), In(b), In(cc), n, Out(32 * n), None) == [exp], op
        io = Out(data=a)
        assert call(cfg, L.msm_amd_fr_map_device, op, layout, k, io, In(b), In(cc), n, io, None) == [exp], op
    layout, a, k, exp = gc.fr_shift_case(n)
    assert call(cfg, L.msm_amd_fr_shift_device, layout, k, In(a), n, Out(32 * n), None) == [exp]
    io = Out(data=a)
    assert call(cfg, L.msm_amd_fr_shift_device, layout, k, io, n, io, None) == [exp]
    layout, a, k, exp = gc.fr_lincomb_case(n)
    assert call(cfg, L.msm_amd_fr_lincomb_device, layout, k, In(a), n, gc.N_VEC, Out(32 * n), None) == [exp]
    io = Out(data=a, writable=[(0, 32 * n)])                           # "out may be the first vector of a": the others stay
    assert call(cfg, L.msm_amd_fr_lincomb_device, layout, k, io, n, gc.N_VEC, io, None)[0][:32 * n] == exp
    layout, a, exp, zeros = gc.fr_inverse_case(n)
    nz = ctypes.c_uint64(99)
    assert call(cfg, L.msm_amd_fr_batch_inverse_device, layout, In(a), n, Out(32 * n), ctypes.byref(nz), None) == [exp]
    assert nz.value == zeros
    io = Out(data=a)
    assert call(cfg, L.msm_amd_fr_batch_inverse_device, layout, io, n, io, None, None) == [exp]


# ---- scans: one tile of 2^kFrTileLog = 512 records +- 1 ---------------------------------------------------------------------------
def scans(c, L, kind, n):
    fn = L.msm_amd_fr_prefix_product_device if kind == "product" else L.msm_amd_fr_prefix_sum_device
    for mode in (0, 1):
        layout, a, exp = gc.fr_scan_case(kind, n, mode)
        assert call(c, fn, layout, mode, In(a), n, gc.N_VEC, Out(len(a)), None) == [exp], (n, mode)
        io = Out(data=a)
        assert call(c, fn, layout, mode, io, n, gc.N_VEC, io, None) == [exp], (n, mode)


@pytest.mark.parametrize("kind", ["product", "sum"])
@pytest.mark.parametrize("n", gc.FR_SCAN_N)
def test_fr_prefix_scans(cfg, L, kind, n):
    scans(cfg, L, kind, n)


@pytest.mark.parametrize("kind", ["product", "sum"])
def test_fr_prefix_scans_tiles_of_four(tiles_of_four, msm_pkg, L, kind):
    """three-, four- and five-level plans: the partial tile of every level lies next to a guard"""
    for n in gc.FR_SCAN_SMALL_TILE_N:
        assert msm_pkg.test_fr_plan(n, gc.N_VEC, 2)["levels"] >= 3
        scans(tiles_of_four, L, kind, n)


@pytest.mark.parametrize("n", gc.FR_SCAN_N)
def test_fr_poly_eval_and_div_linear(cfg, L, n):
    layout, a, z, y, q, rem = gc.fr_poly_case(n)
    nv = gc.N_VEC
    assert call(cfg, L.msm_amd_fr_poly_eval_device, layout, z, In(a), n, nv, HOut(32 * nv), None) == [y]
    assert call(cfg, L.msm_amd_fr_poly_div_linear_device, layout, z, In(a), n, nv, Out(len(a)), HOut(32 * nv), None) == [q, rem]
    assert call(cfg, L.msm_amd_fr_poly_div_linear_device, layout, z, In(a), n, nv, Out(len(a)), None, None) == [q]
    io = Out(data=a)
    assert call(cfg, L.msm_amd_fr_poly_div_linear_device, layout, z, io, n, nv, io, HOut(32 * nv), None) == [q, rem]


# ---- sparse product: rows round one wave (64) and one workgroup (256); d_x read-only -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", gc.MATVEC_ROWS)
def test_fr_matvec(cfg, L, n_rows):
    layout, mat, x, exp = gc.matvec_case(n_rows)
    handle = cfg.fr_matrix_build(*mat.c_args(), layout)
    try:
        assert call(cfg, L.msm_amd_fr_matvec_device, handle.h, layout, In(x), Out(32 * n_rows), None) == [exp]
    finally:
        handle.free()


# ---- multilinear tables: n = 2 .. 1024, both orders, stride = n and stride = n + 3 ---------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "stride_n_plus_3"])
@pytest.mark.parametrize("n", gc.MLE_N)
def test_fr_mle_bind(cfg, L, n, strided):
    """the gap records between the tables, and the records from n/2 up to the stride, are guards too (mle_bind_writable
    quotes the header)"""
    m = n.bit_length() - 1
    fn = L.msm_amd_fr_mle_bind_device
    for order in mle_ref.ORDERS:
        for n_bind in sorted({1, min(2, m), m}):
            layout, stride, data, r, exp = gc.mle_bind_case(n, order, n_bind, strided)
            span = 32 * ((gc.N_VEC - 1) * stride + n // 2)
            out = Out(span, writable=gc.mle_bind_writable(n, stride))
            got, = call(cfg, fn, layout, order, r, n_bind, In(data), n, gc.N_VEC, stride, out, None)
            assert mle_ref.bind_outputs(got, n, n_bind, gc.N_VEC, stride) == exp, (order, n_bind)
    layout, stride, data, r, exp = gc.mle_bind_case(n, mle_ref.HIGH, 1, strided)      # in place is HIGH's alone
    io = Out(data=data, writable=gc.mle_bind_writable(n, stride))
    got, = call(cfg, fn, layout, mle_ref.HIGH, r, 1, io, n, gc.N_VEC, stride, io, None)
    assert mle_ref.bind_outputs(got, n, 1, gc.N_VEC, stride) == exp


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "stride_n_plus_3"])
@pytest.mark.parametrize("n", gc.MLE_N)
def test_fr_mle_eval_eq_table_and_sumcheck_round(cfg, msm_pkg, L, n, strided):
    m = n.bit_length() - 1
    for order in mle_ref.ORDERS:
        layout, stride, data, point, exp = gc.mle_eval_case(n, order, strided)
        got = call(cfg, L.msm_amd_fr_mle_eval_device, layout, order, point, In(data), n, gc.N_VEC, stride, HOut(32 * gc.N_VEC), None)
        assert got == [exp], order
        if not strided:
            layout, point, exp = gc.mle_eq_case(m, order)
            assert call(cfg, L.msm_amd_fr_eq_table_device, layout, order, point, m, Out(32 * n), None) == [exp], order
        for form, n_vec in gc.MLE_ROUND_SHAPES:
            layout, stride, data, exp = gc.mle_round_case(n, order, form, n_vec, strided)
            values = msm_pkg.sumcheck_values(form, n_vec)              # d + 1 records, not the 5 the wrapper passes
            got = call(cfg, L.msm_amd_fr_sumcheck_round_device, layout, order, form, In(data), n, n_vec, stride, HOut(32 * values), None)
            assert got == [exp], (order, form, n_vec)


# ---- transforms: one size per pass geometry, the smallest log_n of each ------------------------------------------------------------
def ntt_sizes(msm_pkg, tile_log, logs):
    seen, sizes = set(), []
    for log_n in logs:
        geo = ntt_shapes.geometry(msm_pkg.test_ntt_plan(log_n, tile_log))
        if not geo <= seen:
            sizes.append(log_n)
            seen |= geo
    return sizes


def ntt_everything(c, L, log_n):
    dom = c.ntt_domain(log_n & 1, log_n)
    try:
        for n_vec in (1, 3):
            for direction in ntt_ref.DIRECTIONS:
                for shifted in (False, True):
                    layout, root, data, shift, exp = gc.ntt_case(log_n, n_vec, direction, shifted)
                    args = (dom.h, direction, layout, shift)
                    assert call(c, L.msm_amd_ntt_device, *args, In(data), Out(len(data)), n_vec, None) == [exp], (log_n, n_vec)
                    io = Out(data=data)
                    assert call(c, L.msm_amd_ntt_device, *args, io, io, n_vec, None) == [exp], (log_n, n_vec)
    finally:
        dom.free()


def test_ntt_default_tile(cfg, msm_pkg, L):
    """one pass up to 2^kNttTileLog = 1024 records: every level count is a geometry of its own"""
    sizes = ntt_sizes(msm_pkg, ntt_shapes.DEFAULT_TILE, range(0, 11))
    assert 10 in sizes and 1 in sizes
    for log_n in sizes:
        ntt_everything(cfg, L, log_n)


def test_ntt_tiles_of_eight(msm_pkg, L, monkeypatch):
    """MSM_AMD_NTT_TILE_LOG = 3: two, three and more passes on at most 512 records"""
    monkeypatch.setenv("MSM_AMD_NTT_TILE_LOG", "3")
    c2 = msm_pkg.setup_metal_state()
    try:
        sizes = ntt_sizes(msm_pkg, 3, range(1, 10))
        assert max(len(msm_pkg.test_ntt_plan(k, 3)) for k in sizes) >= 3
        for log_n in sizes:
            ntt_everything(c2, L, log_n)
    finally:
        c2.close()


@pytest.mark.parametrize("log_n", gc.NTT_POINTS_LOGS)
def test_ntt_points(cfg, L, log_n):
    n = 1 << log_n
    for direction in ntt_ref.DIRECTIONS:
        li, root, data, want = gc.ntt_points_case(log_n, direction)
        dom = cfg.ntt_domain(root, log_n)
        try:
            lo = gc.G1_OUT[log_n % 2]
            exp = gc.point_records(1, lo, want)
            assert call(cfg, L.msm_amd_ntt_points_device, dom.h, direction, li, In(data), lo, Out(len(exp)), None) == [exp]
            prep, = call(cfg, L.msm_amd_ntt_points_device, dom.h, direction, li, In(data), gc.PREPARED, Out(64 * n), None)
            assert affine_of(cfg, 1, prep, n) == gc.point_records(1, 0, want)
            io = Out(data=prep)                                        # in place, PREPARED in and out: the round trip
            back, = call(cfg, L.msm_amd_ntt_points_device, dom.h, 1 - direction, gc.PREPARED, io, gc.PREPARED, io, None)
            assert affine_of(cfg, 1, back, n) == gc.point_records(1, 0, list(gc.ntt_points_inputs(log_n)))
        finally:
            dom.free()


def affine_of(cfg, group, prepared, n):
    """PREPARED records as canonical affine H2C records: [1] P through the multiplication call, which takes them as bases
    (plain buffers: this is no call under test here)"""
    ones = mr.scalars_bytes([1] * n, 0)
    size = gc.PREPARED_BYTES[group]                                    # an H2C affine record is as long as a prepared one
    d_in, d_one, d_out = cfg.alloc(len(prepared)), cfg.alloc(len(ones)), cfg.alloc(size * n)
    try:
        cfg.to_device(d_in, prepared)
        cfg.to_device(d_one, ones)
        cfg.mul_points_device(d_one, d_in, n, d_out, mr.EACH, 0, gc.PREPARED if group == 1 else gc.G2_PREPARED, 0, g2=group == 2)
        return cfg.to_host(d_out, size * n)
    finally:
        for d in (d_in, d_one, d_out):
            cfg.free(d)


# ---- Poseidon: n round one wave (64) and one workgroup (256), every t -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", gc.POSEIDON_T)
def test_poseidon_permute_and_hash(cfg, L, t):
    params = cfg.poseidon_params(t)
    try:
        for n in gc.POSEIDON_N:
            layout, data, exp = gc.poseidon_permute_case(t, n)
            assert call(cfg, L.msm_amd_poseidon_permute_device, params.h, layout, In(data), n, Out(len(data)), None) == [exp], n
            io = Out(data=data)
            assert call(cfg, L.msm_amd_poseidon_permute_device, params.h, layout, io, n, io, None) == [exp], n
            layout, data, tag, exp = gc.poseidon_hash_case(t, n)
            assert call(cfg, L.msm_amd_poseidon_hash_device, params.h, layout, tag, In(data), n, Out(32 * n), None) == [exp], n
            if t == 2:                                                 # "out == in is allowed for t = 2 only"
                io = Out(data=data)
                assert call(cfg, L.msm_amd_poseidon_hash_device, params.h, layout, tag, io, n, io, None) == [exp], n
    finally:
        params.free()


@pytest.mark.parametrize("t,n_leaves", gc.MERKLE_SHAPES)
def test_poseidon_merkle_build_and_paths(cfg, msm_pkg, L, t, n_leaves):
    """leaves read-only in the build; leaves and tree read-only in the paths call"""
    layout, leaves, tag, tree, root, idx, paths = gc.merkle_case(t, n_leaves)
    params = cfg.poseidon_params(t)
    try:
        build = L.msm_amd_poseidon_merkle_build_device
        assert call(cfg, build, params.h, layout, tag, In(leaves), n_leaves, Out(len(tree)), HOut(32), None) == [tree, root]
        assert call(cfg, build, params.h, layout, tag, In(leaves), n_leaves, Out(len(tree)), None, None) == [tree]
        ids = msm_pkg._csr_u64(idx)
        got = call(cfg, L.msm_amd_poseidon_merkle_paths_device, params.h, layout, In(leaves), n_leaves, In(tree), ids, len(idx),
                   Out(len(paths)), None)
        assert got == [paths]
        if (t, n_leaves) == gc.MERKLE_SHAPES[0]:                       # a leaf count that is no power of the arity is refused
            bad_t, bad_n = gc.MERKLE_BAD_LEAVES
            p3 = cfg.poseidon_params(bad_t)
            try:
                call(cfg, build, p3.h, gc.MONT_LE, None, Out(32 * bad_n), bad_n, Out(32 * bad_n), HOut(32), None, ok=msm_pkg.INPUT_ERROR)
            finally:
                p3.free()
    finally:
        params.free()


# ---- lookups --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ["block", "wave", "lane"])
@pytest.mark.parametrize("n_rows", gc.LOOKUP_ROWS)
def test_fr_lookup_build_and_multiplicities(cfg, msm_pkg, L, n_rows, count, monkeypatch):
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    fn = L.msm_amd_fr_lookup_multiplicities_device
    layout, table = gc.lookup_case(n_rows, 1)[:2]
    h = P()
    assert call(cfg, L.msm_amd_fr_lookup_build_device, layout, In(table), n_rows, ctypes.byref(h), None) == []   # the table: read-only
    try:
        for total in gc.LOOKUP_TOTAL:
            layout, table, data, n_vec, m, idx, rep = gc.lookup_case(n_rows, total)
            want_idx = struct.pack("<%dI" % total, *idx)
            report = (ctypes.c_uint64 * 4)()
            args = (h, layout, msm_pkg.LOOKUP_COUNT_MISSING, In(data), total // n_vec, n_vec)
            assert call(cfg, fn, *args, Out(32 * n_rows), Out(4 * total), report, None) == [m, want_idx], total
            assert dict(zip(msm_pkg.LOOKUP_REPORT_FIELDS, report)) == rep
            assert call(cfg, fn, *args, Out(32 * n_rows), None, report, None) == [m], total
        layout, table, data, n_vec, m, idx, rep = gc.lookup_case(n_rows, 257, miss=True)
        want_idx = struct.pack("<257I", *idx)
        with Arena(cfg) as a:                                          # a STRICT miss: m_out AND its guards unchanged
            d_in, d_m, d_idx = a.add("in", data=data, readonly=True), a.add("m", 32 * n_rows), a.add("idx", 4 * 257)
            a.commit()
            report = (ctypes.c_uint64 * 4)()
            st = fn(cfg.h, h, layout, msm_pkg.LOOKUP_STRICT, P(d_in.ptr), 257, 1, P(d_m.ptr), P(d_idx.ptr), report, None)
            assert st == msm_pkg.INPUT_ERROR and report[0] == 1 and report[1] == 256
            a.verify()
            assert a.get("m") == a.filled("m") and a.get("idx") == want_idx      # "written in either mode"
    finally:
        assert L.msm_amd_fr_lookup_free(cfg.h, h) == 0


# ---- points: n = 1, 3, 63, 65, and 255 .. 257 where a kernel launches 256 threads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_check_points(cfg, msm_pkg, L, group):
    """d_reasons is n BYTES: its rear guard is not dword aligned; the points are read-only"""
    fn = L.msm_amd_check_points_device if group == 1 else L.msm_amd_g2_check_points_device
    for n in gc.check_sizes(group):
        layout, checks, data, reasons, report = gc.check_case(group, n)
        rep = msm_pkg.CheckReport()
        assert call(cfg, fn, layout, In(data), n, checks, Out(n), ctypes.byref(rep)) == [reasons], n
        assert c.same_report(rep.as_dict(), report)
        assert call(cfg, fn, layout, In(data), n, checks, None, ctypes.byref(rep)) == []
        assert c.same_report(rep.as_dict(), report)


@pytest.mark.parametrize("group", [1, 2])
def test_decompress_and_compress_points(cfg, msm_pkg, L, group):
    dec = L.msm_amd_decompress_points_device if group == 1 else L.msm_amd_g2_decompress_points_device
    com = L.msm_amd_compress_points_device if group == 1 else L.msm_amd_g2_compress_points_device
    prepared = gc.PREPARED if group == 1 else gc.G2_PREPARED
    for n in gc.COMPRESS_N:
        for fmt in gc.FORMATS:
            data, recs, reasons, report, outs = gc.decompress_case(group, n, fmt)
            for lo, want in outs.items():
                rep = msm_pkg.DecompressReport()
                assert call(cfg, dec, fmt, In(data), n, lo, Out(len(want)), Out(n), ctypes.byref(rep)) == [want, reasons], (n, fmt, lo)
                assert cr.same_report(rep.as_dict(), report)
                assert call(cfg, dec, fmt, In(data), n, lo, Out(len(want)), None, ctypes.byref(rep)) == [want]
                pts, want_c, n_bad = gc.compress_case(group, n, fmt, lo)
                bad = ctypes.c_uint64(77)
                assert call(cfg, com, lo, In(pts), n, fmt, Out(len(want_c)), ctypes.byref(bad)) == [want_c], (n, fmt, lo)
                assert bad.value == n_bad
            rep = msm_pkg.DecompressReport()
            prep, rs = call(cfg, dec, fmt, In(data), n, prepared, Out(gc.PREPARED_BYTES[group] * n), Out(n), ctypes.byref(rep))
            assert rs == reasons and cr.same_report(rep.as_dict(), report)
            pts = [cr.decode(group, fmt, r)[1] for r in recs]          # an invalid record becomes the identity
            assert affine_of(cfg, group, prep, n) == gc.point_records(group, 0, pts), (n, fmt)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("mode", [mr.EACH, mr.ONE])
def test_mul_points(cfg, L, group, mode):
    fn = L.msm_amd_mul_points_device if group == 1 else L.msm_amd_g2_mul_points_device
    prepared = gc.PREPARED if group == 1 else gc.G2_PREPARED
    for n in gc.mul_sizes(group):
        sl, li, scalars, pts, want = gc.mul_case(group, n, mode)
        for lo in gc.mul_out_layouts(group, n):
            exp = gc.point_records(group, lo, want)
            assert call(cfg, fn, sl, li, mode, In(scalars), In(pts), n, lo, Out(len(exp))) == [exp], (n, lo)
        prep, = call(cfg, fn, sl, li, mode, In(scalars), In(pts), n, prepared, Out(gc.PREPARED_BYTES[group] * n))
        assert affine_of(cfg, group, prep, n) == gc.point_records(group, 0, want), n


@pytest.mark.parametrize("group", [1, 2])
def test_bases_prepare(cfg, L, group):
    """through lib(), because the wrapper allocates d_prepared itself"""
    fn = L.msm_amd_bases_prepare_device if group == 1 else L.msm_amd_g2_bases_prepare_device
    for n in gc.PREPARE_N:
        layout = gc.layout_of(group, n)
        _, pts = gc.group_points(group, n, 830 + n)
        data = b"".join(mr.base_record(group, layout, p, 7 + i) for i, p in enumerate(pts))
        prep, = call(cfg, fn, layout, In(data), n, Out(gc.PREPARED_BYTES[group] * n))
        assert affine_of(cfg, group, prep, n) == gc.point_records(group, 0, pts), n


# ---- sort: in place -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits", [32, 12])
def test_sort_pairs(cfg, L, key_bits):
    for n_pairs in gc.SORT_N:
        data, want = gc.sort_case(n_pairs, key_bits)
        io = Out(data=data)
        got, = call(cfg, L.msm_amd_sort_pairs_device, io, n_pairs, key_bits, None)
        assert list(struct.iter_unpack("<II", got)) == want, n_pairs              # the sort is stable


# ---- pairings ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups,group_size", gc.PAIRING_SHAPES)
def test_pairing_product_and_final_exponentiation(cfg, L, n_groups, group_size):
    """d_is_one is n_groups BYTES; the points are read-only; a MILLER_ONLY record is a representative, read through the
    final exponentiation"""
    l1, l2, a, b, want, one = gc.pairing_case(n_groups, group_size)
    fn, fe = L.msm_amd_pairing_product_device, L.msm_amd_final_exponentiation_device
    for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
        exp = gc.gt_records(want, gt)
        args = (l1, l2, In(a), In(b), n_groups, group_size)
        assert call(cfg, fn, *args, 0, gt, Out(len(exp)), Out(n_groups), None) == [exp, one], gt
        assert call(cfg, fn, *args, 0, gt, Out(len(exp)), None, None) == [exp], gt
        mil, = call(cfg, fn, *args, pr.PAIRING_MILLER_ONLY, gt, Out(len(exp)), None, None)
        assert call(cfg, fe, gt, In(mil), n_groups, Out(len(exp)), Out(n_groups), None) == [exp, one], gt
        io = Out(data=mil)
        assert call(cfg, fe, gt, io, n_groups, io, None, None) == [exp], gt


# ---- MSM: the device inputs are gathered "in place" -- they are only read; the result is 96 / 192 bytes of host memory ------------------
@pytest.mark.parametrize("n", gc.MSM_N)
def test_msm_inputs_are_only_read(cfg, msm_pkg, L, n):
    sl, scalars, pts, want = gc.msm_case(1, n)
    out, = call(cfg, L.msm_amd_msm_device, sl, 0, In(scalars), In(pts), n, HOut(96))
    assert gc.msm_result(1, out) == want
    bits, stats = ctypes.c_uint32(0), (ctypes.c_uint64 * 4)()
    assert call(cfg, L.msm_amd_scalar_width_device, sl, In(scalars), n, 0, ctypes.byref(bits), stats) == []
    words = [k % gc.R for k in fr_words(scalars, sl)]
    assert bits.value == max(w.bit_length() for w in words) and stats[0] == words.count(0)
    with Arena(cfg) as a, HostArena() as host:                         # a batch of two instances over the same buffers
        d_s, d_p = a.add("scalars", data=scalars, readonly=True), a.add("points", data=pts, readonly=True)
        res = host.add("out", 2 * 96)
        a.commit()
        host.commit()
        sp, pp, nn = (P * 2)(d_s.ptr, d_s.ptr), (P * 2)(d_p.ptr, d_p.ptr), (ctypes.c_size_t * 2)(n, n)
        assert L.msm_amd_msm_batch_device(cfg.h, sl, 0, 2, sp, pp, nn, P(res.ptr)) == 0
        a.verify()
        host.verify()
        assert host.get("out") == out + out
    sl, scalars, pts, want = gc.msm_case(1, n, bits=20)
    out, = call(cfg, L.msm_amd_msm_bounded_device, sl, 0, In(scalars), In(pts), n, 20, 0, HOut(96))
    assert gc.msm_result(1, out) == want
    sl, scalars, pts, want = gc.msm_case(2, n)
    out, = call(cfg, L.msm_amd_msm_g2_device, sl, 0, In(scalars), In(pts), n, HOut(192))
    assert gc.msm_result(2, out) == want
    sl, scalars, pts, want = gc.msm_case(2, n, bits=20)
    out, = call(cfg, L.msm_amd_msm_g2_bounded_device, sl, 0, In(scalars), In(pts), n, 20, 0, HOut(192))
    assert gc.msm_result(2, out) == want


def fr_words(scalars, layout):
    import fr_ref
    return fr_ref.decode(scalars, layout)


# ---- refused calls write nothing: one INPUT_ERROR per family, and a busy ctx ----------------------------------------------------------
def test_refused_calls_leave_the_whole_arena_unchanged(cfg, msm_pkg, L):
    bad = msm_pkg.INPUT_ERROR
    n = 65
    layout, a, k, _ = gc.fr_shift_case(n)
    io, out = Out(data=a), Out(32 * n)
    call(cfg, L.msm_amd_fr_shift_device, layout, k, In(a), n, At(out, 8), None, ok=bad)             # misaligned
    call(cfg, L.msm_amd_fr_shift_device, layout, k, io, n - 1, At(io, 32), None, ok=bad)            # partial overlap
    call(cfg, L.msm_amd_fr_map_device, 6, layout, k, In(a), In(a), In(a), n, Out(32 * n), None, ok=bad)   # no seventh op
    io = Out(data=a)
    call(cfg, L.msm_amd_fr_prefix_sum_device, layout, 0, io, n - 1, 1, At(io, 32), None, ok=bad)    # partial overlap
    call(cfg, L.msm_amd_fr_poly_eval_device, 2, k, In(a), n, 1, HOut(32), None, ok=bad)             # CANON_BE32 is refused
    call(cfg, L.msm_amd_fr_eq_table_device, layout, 0, k, 1, At(Out(96), 8), None, ok=bad)          # misaligned
    lay, stride, data, r, _ = gc.mle_bind_case(64, mle_ref.LOW, 1, False)
    io = Out(data=data)
    call(cfg, L.msm_amd_fr_mle_bind_device, lay, mle_ref.LOW, r, 1, io, 64, gc.N_VEC, stride, io, None, ok=bad)   # LOW in place
    lay, mat, x, _ = gc.matvec_case(63)
    handle = cfg.fr_matrix_build(*mat.c_args(), lay)
    try:
        io = Out(32 * 100, data=x)
        call(cfg, L.msm_amd_fr_matvec_device, handle.h, lay, io, At(io, 32), None, ok=bad)          # y overlaps x
    finally:
        handle.free()
    lay, root, data, shift, _ = gc.ntt_case(6, 1, 0, False)
    dom = cfg.ntt_domain(root, 6)
    try:
        io = Out(2 * len(data), data=data)
        call(cfg, L.msm_amd_ntt_device, dom.h, 0, lay, None, io, At(io, 32), 1, None, ok=bad)       # partial overlap
        li, root_p, pdata, _ = gc.ntt_points_case(6, 0)
        call(cfg, L.msm_amd_ntt_points_device, dom.h, 0, li, In(pdata), 9, Out(64 * 64), None, ok=bad)   # unknown layout
    finally:
        dom.free()
    params = cfg.poseidon_params(3)
    try:
        lay, data, tag, _ = gc.poseidon_hash_case(3, 63)
        io = Out(data=data)
        call(cfg, L.msm_amd_poseidon_hash_device, params.h, lay, tag, io, 63, io, None, ok=bad)     # in place with t = 3
    finally:
        params.free()
    lay, table, data, _, _, _, _ = gc.lookup_case(63, 255)
    lookup = cfg.fr_lookup_build(table, lay)
    try:
        report = (ctypes.c_uint64 * 4)()
        call(cfg, L.msm_amd_fr_lookup_multiplicities_device, lookup.h, lay, msm_pkg.LOOKUP_COUNT_MISSING, In(data), 255, 1, Out(32 * 63),
             At(Out(4 * 256), 2), report, None, ok=bad)                                             # d_idx_out must be 4-byte aligned
    finally:
        lookup.free()
    layout, checks, data, _, _ = gc.check_case(1, 63)
    rep = msm_pkg.CheckReport()
    call(cfg, L.msm_amd_check_points_device, 9, In(data), 63, checks, Out(63), ctypes.byref(rep), ok=bad)          # unknown layout
    data, _, _, _, _ = gc.decompress_case(1, 63, 0)
    drep = msm_pkg.DecompressReport()
    call(cfg, L.msm_amd_decompress_points_device, 0, In(data), 63, msm_pkg.POINT_JAC_BE32, Out(96 * 63), Out(63), ctypes.byref(drep), ok=bad)
    pts, _, _ = gc.compress_case(2, 63, 0, 0)
    call(cfg, L.msm_amd_g2_compress_points_device, 9, In(pts), 63, 0, Out(64 * 63), ctypes.byref(ctypes.c_uint64(0)), ok=bad)
    sl, li, scalars, pts, _ = gc.mul_case(1, 63, mr.EACH)
    call(cfg, L.msm_amd_mul_points_device, sl, li, 2, In(scalars), In(pts), 63, 0, Out(64 * 63), ok=bad)            # no third base mode
    l1, l2, a1, b2, _, _ = gc.pairing_case(3, 1)
    call(cfg, L.msm_amd_pairing_product_device, l1, l2, In(a1), In(b2), 3, 1, pr.PAIRING_MILLER_ONLY, 0, Out(3 * 384), Out(3), None,
         ok=bad)                                                                                                   # is_one with MILLER_ONLY
    call(cfg, L.msm_amd_final_exponentiation_device, 2, In(bytes(384)), 1, Out(384), Out(1), None, ok=bad)         # unknown GT layout
    sl, scalars, pts, _ = gc.msm_case(1, 65)
    call(cfg, L.msm_amd_msm_device, 9, 0, In(scalars), In(pts), 65, HOut(96), ok=bad)                              # unknown scalar layout
    sl, scalars, pts, _ = gc.msm_case(1, 65)                            # a record beyond the bound: "the output is left untouched"
    call(cfg, L.msm_amd_msm_bounded_device, sl, 0, In(scalars), In(pts), 65, 20, 0, HOut(96), ok=bad)


def test_a_busy_ctx_refuses_and_writes_nothing(msm_pkg, L):
    """test_hold keeps the ctx busy (the hold kernel carries its own time limit); the bounded wait of a call then runs out"""
    c2 = msm_pkg.setup_metal_state()
    layout, a, k, exp = gc.fr_shift_case(257)
    try:
        with Arena(c2) as arena:
            d_a, d_out = arena.add("a", data=a, readonly=True), arena.add("out", len(a))
            arena.commit()
            c2.set_wait_timeout_ms(150)
            hold = c2.test_hold(4000)
            st = L.msm_amd_fr_shift_device(c2.h, layout, k, P(d_a.ptr), 257, P(d_out.ptr), None)
            st2 = L.msm_amd_fr_prefix_sum_device(c2.h, layout, 0, P(d_a.ptr), 257, 1, P(d_out.ptr), None)
            c2.test_release(hold)
            c2.set_wait_timeout_ms(60000)
            c2.synchronize()
            assert st == msm_pkg.PIPELINE_ERROR and st2 == msm_pkg.PIPELINE_ERROR
            arena.unchanged()
            assert L.msm_amd_fr_shift_device(c2.h, layout, k, P(d_a.ptr), 257, P(d_out.ptr), None) == 0     # and works again
            assert arena.verify().get("out") == exp
    finally:
        c2.close()


# ---- the host-buffer forms of the ctx calls whose copy-back could be rounded up -------------------------------------------------------
def test_host_buffer_forms_copy_back_exactly(cfg, msm_pkg, L):
    """outputs whose length is no multiple of 16 (reasons, is_one, idx with n odd, the 96-byte result) or small (y_out,
    g_out, root32), in a HostArena"""
    H = In                                                             # one HostArena holds everything
    for group, fn in ((1, L.msm_amd_check_points), (2, L.msm_amd_g2_check_points)):
        for n in (3, 65):
            layout, checks, data, reasons, report = gc.check_case(group, n)
            rep = msm_pkg.CheckReport()
            assert host_call(cfg, fn, layout, H(data), n, checks, Out(n), ctypes.byref(rep)) == [reasons], (group, n)
    for n in (3, 65):
        data, _, reasons, report, outs = gc.decompress_case(1, n, 0)
        rep = msm_pkg.DecompressReport()
        for lo, want in outs.items():
            assert host_call(cfg, L.msm_amd_decompress_points, 0, H(data), n, lo, Out(len(want)), Out(n), ctypes.byref(rep)) == [want, reasons]
            pts, want_c, n_bad = gc.compress_case(1, n, 0, lo)
            bad = ctypes.c_uint64(0)
            assert host_call(cfg, L.msm_amd_compress_points, lo, H(pts), n, 0, Out(32 * n), ctypes.byref(bad)) == [want_c]
    for n_groups, group_size in ((3, 1), (3, 5)):
        l1, l2, a, b, want, one = gc.pairing_case(n_groups, group_size)
        exp = gc.gt_records(want, 0)
        assert host_call(cfg, L.msm_amd_pairing_product, l1, l2, H(a), H(b), n_groups, group_size, 0, 0, Out(len(exp)), Out(n_groups)) == [exp, one]
    layout, table, data, n_vec, m, idx, rep = gc.lookup_case(65, 257)
    handle = cfg.fr_lookup_build(table, layout)
    try:
        report = (ctypes.c_uint64 * 4)()
        got = host_call(cfg, L.msm_amd_fr_lookup_multiplicities, handle.h, layout, msm_pkg.LOOKUP_COUNT_MISSING, H(data), 257, 1,
                        Out(32 * 65), Out(4 * 257), report)
        assert got == [m, struct.pack("<257I", *idx)]
    finally:
        handle.free()
    sl, scalars, pts, want = gc.msm_case(1, 65)
    out, = host_call(cfg, L.msm_amd_msm, sl, 0, H(scalars), H(pts), 65, Out(96))
    assert gc.msm_result(1, out) == want
    layout, a, z, y, q, rem = gc.fr_poly_case(513)
    assert host_call(cfg, L.msm_amd_fr_poly_eval, layout, z, H(a), 513, gc.N_VEC, Out(32 * gc.N_VEC)) == [y]
    for form, n_vec in gc.MLE_ROUND_SHAPES:
        layout, stride, data, exp = gc.mle_round_case(128, mle_ref.LOW, form, n_vec, True)
        values = msm_pkg.sumcheck_values(form, n_vec)
        assert host_call(cfg, L.msm_amd_fr_sumcheck_round, layout, mle_ref.LOW, form, H(data), 128, n_vec, stride, Out(32 * values)) == [exp]
    t, n_leaves = 3, 64
    layout, leaves, tag, tree, root, idx, paths = gc.merkle_case(t, n_leaves)
    params = cfg.poseidon_params(t)
    try:
        got = host_call(cfg, L.msm_amd_poseidon_merkle_build, params.h, layout, tag, H(leaves), n_leaves, Out(len(tree)), Out(32))
        assert got == [tree, root]
    finally:
        params.free()
