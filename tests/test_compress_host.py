"""Host tests (no GPU) of the compressed point formats: the host twins of decompress / compress against the big-integer
model of compress_ref byte for byte, the round trips, the raw-limb root ops, argument errors, the planted cases."""
import ctypes
import os
import random

import pytest

import check_ref as c
import compress_ref as r
import g2_ref as g
import test_g2_host as th

SIZES = [1, 63, 64, 65, 257]
FORMATS = [r.ARK, r.PARITY]
LAYOUTS = {1: (c.H2C, c.ARK_AFFINE), 2: (c.G2_H2C, c.G2_ARK)}
_ENC = {}


def encoded(group, fmt, n):
    """n valid points (a progression), compressed by the model; computed once"""
    key = (group, fmt, n)
    if key not in _ENC:
        pts = r.points(group, 257, 11 + group)
        _ENC[key] = ([r.encode(group, fmt, p) for p in pts[:n]], pts[:n])
    return _ENC[key]


def test_new_symbols_and_constants(msm_pkg):
    L = msm_pkg.lib()
    for name in ("msm_amd_decompress_points", "msm_amd_g2_decompress_points_device", "msm_amd_host_decompress_points",
                 "msm_amd_host_g2_decompress_points", "msm_amd_compress_points", "msm_amd_g2_compress_points_device",
                 "msm_amd_host_compress_points", "msm_amd_host_g2_compress_points", "msm_amd_compressed_bytes"):
        assert hasattr(L, name) and name in msm_pkg.EXPORTS
    assert (msm_pkg.COMPRESSED_ARK, msm_pkg.COMPRESSED_PARITY, msm_pkg.POINT_BAD_ENCODING) == (0, 1, 4)
    assert (msm_pkg.RAW_FE_SQRT, msm_pkg.G2_RAW_FQ2_SQRT) == (36, 10)
    assert [msm_pkg.compressed_bytes(f, grp) for f in (0, 1) for grp in (1, 2)] == [32, 64, 32, 64]
    assert msm_pkg.compressed_bytes(2, 1) == 0 and msm_pkg.compressed_bytes(0, 3) == 0 and msm_pkg.compressed_bytes(0, 0) == 0
    assert ctypes.sizeof(msm_pkg.DecompressReport) == 64


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", SIZES)
def test_host_twin_against_model(msm_pkg, group, fmt, n):
    rng = random.Random(1000 * group + 10 * n + fmt)
    good, _ = encoded(group, fmt, n)
    cases, names = r.case_records(group, fmt, n)
    buf, placed = r.plant(b"".join(good), r.SIZE[group], cases, n, rng)
    recs = [buf[i * r.SIZE[group]:(i + 1) * r.SIZE[group]] for i in range(n)]
    want_rep, want_reasons = r.expected_report(group, fmt, recs)
    for layout in LAYOUTS[group]:
        for threads in (1, 3):
            out, rep, reasons = msm_pkg.host_decompress_points(buf, n, fmt, layout, g2=group == 2, threads=threads)
            assert reasons == want_reasons
            assert out == r.expected_output(group, fmt, layout, recs)
            assert r.same_report(rep, want_rep), (rep, want_rep)
            assert rep["device_ms"] == 0
    out, rep, reasons = msm_pkg.host_decompress_points(buf, n, fmt, LAYOUTS[group][0], g2=group == 2, reasons=False)
    assert reasons is None and r.same_report(rep, want_rep)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_planted_case(msm_pkg, group, fmt):
    cases, names = r.case_records(group, fmt, 7)
    want = {nm: r.expected_reason(group, fmt, rec) for nm, rec in zip(names, cases)}
    # what the model must say about the constructed offenders (the rest is "whatever the model says")
    for nm, reason in want.items():
        if "both flag" in nm or "identity flag with" in nm:
            assert reason == r.BAD_ENCODING, nm
        if nm in ("x = p", "x = p + 1", "x = 2^254 - 1") or nm.startswith(("c0 = ", "c1 = ")):
            assert reason == r.NOT_REDUCED, nm
        if "right-hand side" in nm:
            assert reason == r.NOT_ON_CURVE, nm
        if nm in ("P", "-P", "generator", "-generator", "EIP-196 2 G", "EIP-197 generator", "identity",
                  "curve point outside G2", "G2 point + cofactor point"):
            assert reason == r.VALID, nm
    assert cases[0] != cases[1] and cases[0][:-1] == cases[1][:-1]              # P and -P differ in the flag alone
    data = b"".join(cases)
    out, rep, reasons = msm_pkg.host_decompress_points(data, len(cases), fmt, LAYOUTS[group][0], g2=group == 2)
    assert {nm: reasons[i] for i, nm in enumerate(names)} == want
    assert rep["by_reason"][3] == 0 and rep["n_identity"] == 1
    size = len(out) // len(cases)
    p, minus_p = (out[i * size:(i + 1) * size] for i in (0, 1))
    half = size // 2
    assert p[:half] == minus_p[:half] and p[half:] != minus_p[half:]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trips(msm_pkg, group, fmt):
    n = 65
    good, pts = encoded(group, fmt, n)
    data = b"".join(good[:-1]) + r.encode(group, fmt, None)                     # the identity at the last index
    pts = pts[:-1] + [None]
    for layout in LAYOUTS[group]:
        out, rep, _ = msm_pkg.host_decompress_points(data, n, fmt, layout, g2=group == 2)
        assert rep["n_invalid"] == 0 and rep["n_identity"] == 1
        assert out == b"".join(r.out_record(group, layout, p) for p in pts)
        back, bad = msm_pkg.host_compress_points(out, n, fmt, layout, g2=group == 2)      # compress o decompress
        assert back == data and bad == 0
        again, rep2, _ = msm_pkg.host_decompress_points(back, n, fmt, layout, g2=group == 2)   # decompress o compress
        assert again == out


@pytest.mark.parametrize("group", [1, 2])
def test_compress_bad_and_identity_records(msm_pkg, group):
    pts = r.points(group, 4, 3)
    for layout in LAYOUTS[group]:
        mk = c.g1_rec if group == 1 else c.g2_rec
        recs = [mk(layout, pts[0]), mk(layout, None), c.non_reduced(mk(layout, pts[1]), 0),
                c.non_reduced(mk(layout, pts[2]), len(mk(layout, pts[2]).coords) - 1, top=True), mk(layout, pts[3])]
        if layout in (c.ARK_AFFINE, c.G2_ARK) and (group == 2) == (layout == c.G2_ARK):
            recs.append(c.Rec(group, layout, [c.MAX256] * len(recs[0].coords), flag=1))     # flagged: identity, not bad
        for fmt in FORMATS:
            want = [r.compress_expected(group, fmt, rec) for rec in recs]
            out, bad = msm_pkg.host_compress_points(c.encode_all(recs), len(recs), fmt, layout, g2=group == 2, threads=2)
            assert out == b"".join(w[0] for w in want) and bad == sum(w[1] for w in want) == 2
            assert out[2 * r.SIZE[group]:3 * r.SIZE[group]] == b"\xff" * r.SIZE[group]
            assert r.expected_reason(group, fmt, b"\xff" * r.SIZE[group]) == r.BAD_ENCODING   # no valid encoding


def test_argument_errors(msm_pkg):
    L, IE = msm_pkg.lib(), msm_pkg.INPUT_ERROR
    rep = msm_pkg.DecompressReport()
    buf, out = ctypes.create_string_buffer(64 * 4), ctypes.create_string_buffer(136 * 4)
    ok = [(L.msm_amd_host_decompress_points, (c.H2C, c.ARK_AFFINE), (msm_pkg.POINT_ARK_PROJECTIVE, msm_pkg.POINT_JAC_BE32,
                                                                     msm_pkg.POINT_PREPARED, msm_pkg.POINT_TABLES, 9, -1)),
          (L.msm_amd_host_g2_decompress_points, (0, 1), (msm_pkg.G2_POINT_PREPARED, msm_pkg.G2_POINT_TABLES, 9, -1))]
    for fn, good, bad in ok:
        for layout in good:
            assert fn(0, buf, 4, layout, 1, out, None, ctypes.byref(rep)) == msm_pkg.OK
        for layout in bad:
            assert fn(0, buf, 4, layout, 1, out, None, ctypes.byref(rep)) == IE
        for fmt in (2, -1):
            assert fn(fmt, buf, 4, good[0], 1, out, None, ctypes.byref(rep)) == IE
        assert fn(0, None, 4, good[0], 1, out, None, ctypes.byref(rep)) == IE
        assert fn(0, buf, 4, good[0], 1, None, None, ctypes.byref(rep)) == IE
        assert fn(0, buf, 4, good[0], 1, out, None, None) == IE
        assert fn(0, buf, 1 << 32, good[0], 1, out, None, ctypes.byref(rep)) == IE
        assert fn(0, None, 0, good[0], 1, None, None, ctypes.byref(rep)) == msm_pkg.OK      # n == 0: an empty report
        assert rep.as_dict()["first_invalid"] is None and list(rep.by_reason) == [0] * 5 and rep.n_checked == 0
    bad_n = ctypes.c_uint64(7)
    for fn, good, bad in ((L.msm_amd_host_compress_points, (c.H2C, c.ARK_AFFINE), (1, 3, 4, 5, 9)),
                          (L.msm_amd_host_g2_compress_points, (0, 1), (2, 3, 9))):
        for layout in good:
            assert fn(layout, out, 4, 1, 1, buf, None) == msm_pkg.OK                        # n_bad may be NULL
        for layout in bad:
            assert fn(layout, out, 4, 1, 1, buf, ctypes.byref(bad_n)) == IE
        assert fn(good[0], out, 4, 2, 1, buf, ctypes.byref(bad_n)) == IE
        assert fn(good[0], None, 4, 0, 1, buf, ctypes.byref(bad_n)) == IE
        assert fn(good[0], out, 4, 0, 1, None, ctypes.byref(bad_n)) == IE
        assert fn(good[0], out, 1 << 32, 0, 1, buf, ctypes.byref(bad_n)) == IE
        assert fn(good[0], None, 0, 0, 1, None, ctypes.byref(bad_n)) == msm_pkg.OK and bad_n.value == 0
        bad_n.value = 7


# ---- the raw-limb root ops ------------------------------------------------------------------------------------------------
def fq_sqrt_inputs(seed=5):
    ops = r.fq_sqrt_operands(seed)
    return ops, [w for a, lift in ops for w in r.fq_sqrt_record(a, lift)]


def check_fq_sqrt(ops, out):
    for k, (a, lift) in enumerate(ops):
        w = out[40 * k:40 * k + 40]
        want = c.sqrt_fq(a)
        assert w[9] == (want is not None), (a, lift)
        assert not any(w[10:])
        if want is None:
            assert not any(w[:9])
        else:
            got = g.value(w[:9]) * g.RHO_INV % r.P
            assert got in (want, -want % r.P) and got * got % r.P == a
            assert g.value(w[:9]) < 1.05 * r.P and all(x < (1 << 29) for x in w[:8])       # the stated result bound


def fq2_sqrt_inputs(seed=6):
    rng = random.Random(seed)
    ops = r.fq2_sqrt_operands(seed)
    return ops, [w for a in ops for w in r.fq2_sqrt_record(a, rng)]


def check_fq2_sqrt(ops, out):
    n_roots = 0
    for k, a in enumerate(ops):
        w = out[80 * k:80 * k + 80]
        want = c.sqrt_fq2(a)
        assert w[72] == (want is not None), a
        if want is None:
            assert not any(w)
        else:
            got = g.fq2_of(w[:18])
            assert g.mul2(got, got) == a and got in (want, g.neg2(want))
            n_roots += 1
    return n_roots


def test_raw_fq_sqrt_host(msm_pkg):
    ops, a = fq_sqrt_inputs()
    assert (0, 0) in ops and (1, 0) in ops and (r.P - 1, 0) in ops and (4, 1) in ops and (4, 3) in ops
    assert c.sqrt_fq(r.P - 1) is None
    check_fq_sqrt(ops, msm_pkg.test_op_raw_host(msm_pkg.RAW_FE_SQRT, a, [0] * len(a), len(ops)))


def test_raw_fq2_sqrt_host(msm_pkg):
    ops, a = fq2_sqrt_inputs()
    assert c.sqrt_fq2(ops[1]) is not None and ops[1][1] == 0 and c.sqrt_fq(ops[1][0]) is None     # (non-residue, 0)
    assert {c.sqrt_fq2(ops[2]) is None, c.sqrt_fq2(ops[3]) is None} == {False}                    # (0, t): always a root
    n5, n6 = (c.sqrt_fq(v * v % r.P) for v in (ops[5][0], ops[6][0]))
    assert (ops[5][0] + n5) % r.P == 0 or (ops[6][0] + n6) % r.P == 0                           # a0 + n = 0 is met
    roots = check_fq2_sqrt(ops, msm_pkg.test_op_g2_host(msm_pkg.G2_RAW_FQ2_SQRT, a, [0] * len(a), len(ops)))
    assert roots == 7 + 64


def test_root_ops_keep_their_neighbours_refused(msm_pkg):
    with pytest.raises(msm_pkg.MsmError):
        msm_pkg.test_op_raw_host(37, [0] * 36, [0] * 36, 1)
    with pytest.raises(msm_pkg.MsmError):
        msm_pkg.test_op_g2_host(11, [0] * 72, [0] * 72, 1)


def test_compress_kernels_use_no_scratch():
    """the code object of k_compress.hip, read the way test_g2_host reads k_g2's"""
    kernels = th.kernel_scratch(os.path.join(th.CSRC, "k_compress.o"))
    ours = {k: v for k, v in kernels.items() if "compress_g1_kernel" in k or "compress_g2_kernel" in k}
    assert len(ours) == 4, kernels
    assert all(v == 0 for v in ours.values()), ours
