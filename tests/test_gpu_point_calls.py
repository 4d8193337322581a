"""GPU test of what the point calls share: check, decompress, compress and mul_points of one group run through one
driver and one set of buffers and counters per group.  On ONE ctx, in a fixed order, every call is compared byte for
byte with its host twin (reports as dicts without device_ms): a call must not see the counters, reason bytes or staging
of the call before it, and none of them may touch the workspaces of the MSMs.  The sizes 1, 63, 64, 65 and 257 are the
wave (64) and workgroup (256; the G2 check: 64) edges, 17 is the normalisation group of mul_points plus one."""
import ctypes

import pytest

import check_ref as c
import compress_ref as r
import fr_ref as f
import g2_ref as g
import mul_ref as m
import ntt_ref as t

pytestmark = pytest.mark.gpu

o = c.o


def drop_ms(rep):
    return {k: v for k, v in rep.items() if k != "device_ms"}


def valid_points(msm_pkg, group, n):
    if group == 1:
        return msm_pkg.generate_instance_host(o.SEED_BASE + 77, n)[0]
    return msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(90001, g.GEN2)), g.encode_h2c(g.scalar_mul(7919, g.GEN2)), n)


def planted(buf, stride, recs):
    out = bytearray(buf)
    for i, rec in recs.items():
        out[i * stride:(i + 1) * stride] = rec
    return bytes(out)


def offenders(group):
    """three invalid records of the halo2curves layout: a coordinate + p, off the curve, and (G2) outside the subgroup
    (G1, which has no such points: the other coordinate all ones)"""
    if group == 1:
        good = c.g1_rec(c.H2C, c.g1_points(1, 3)[0])
        third = c.non_reduced(good, 1, top=True)
    else:
        good = c.g2_rec(c.G2_H2C, g.GEN2)
        third = c.g2_rec(c.G2_H2C, c.special_g2()["g2_plus_cofactor"])
    return [c.non_reduced(good, 0), good.with_coord(1, (good.coords[1] + 1) % c.P), third]


def point_calls(cfg, msm_pkg, group):
    """steps 1 to 5 for one group"""
    g2 = group == 2
    stride, checks = (128, 3) if g2 else (64, 1)
    n_check, n_dec = (65, 64) if g2 else (257, 65)
    check = cfg.g2_check_points if g2 else cfg.check_points
    host_check = msm_pkg.host_g2_check_points if g2 else msm_pkg.host_check_points
    layout = c.G2_H2C if g2 else c.H2C

    # 1. check with reasons: three offenders, one per wave / workgroup edge
    at = (0, 63, 64) if g2 else (0, 64, 256)
    bad = offenders(group)
    buf = planted(valid_points(msm_pkg, group, n_check), stride, {i: rec.encode() for i, rec in zip(at, bad)})
    rep, reasons = check(buf, n_check, checks=checks, point_layout=layout)
    h_rep, h_reasons = host_check(buf, n_check, checks=checks, point_layout=layout)
    assert reasons == h_reasons and drop_ms(rep) == drop_ms(h_rep)
    assert [reasons[i] for i in at] == [c.expected_reason(rec, checks) for rec in bad] and reasons.count(0) == n_check - 3
    assert rep["n_invalid"] == 3 and rep["first_invalid"] == 0 and rep["first_reason"] == 1

    # 2. decompress: one BAD_ENCODING record, the last one -- stale counters or a key decoded with the check's old shift
    #    would report another index or reason
    pts = valid_points(msm_pkg, group, n_dec)
    data, n_bad = msm_pkg.host_compress_points(pts, n_dec, r.ARK, layout, g2=g2)
    assert n_bad == 0
    both_flags = r.raw_record(group, 5 if group == 1 else (5, 7), 0xC0)
    data = planted(data, r.SIZE[group], {n_dec - 1: both_flags})
    out, rep, reasons = cfg.decompress_points(data, n_dec, r.ARK, layout, g2=g2)
    h_out, h_rep, h_reasons = msm_pkg.host_decompress_points(data, n_dec, r.ARK, layout, g2=g2)
    assert out == h_out and reasons == h_reasons and drop_ms(rep) == drop_ms(h_rep)
    assert rep["first_invalid"] == n_dec - 1 and rep["first_reason"] == 4 and rep["n_invalid"] == 1
    assert rep["by_reason"] == [n_dec - 1, 0, 0, 0, 1] and out[:(n_dec - 1) * stride] == pts[:(n_dec - 1) * stride]

    # 3. check again, one valid record: a clean report, and exactly one reason byte written
    fn = msm_pkg.lib().msm_amd_g2_check_points if g2 else msm_pkg.lib().msm_amd_check_points
    one, raw_rep, two_bytes = valid_points(msm_pkg, group, 1), msm_pkg.CheckReport(), ctypes.create_string_buffer(b"\xAA\xAA", 2)
    assert fn(cfg.h, layout, one, 1, checks, two_bytes, ctypes.byref(raw_rep)) == msm_pkg.OK
    assert raw_rep.n_invalid == 0 and raw_rep.first_invalid == 0xFFFFFFFFFFFFFFFF and two_bytes.raw == b"\x00\xAA"
    assert drop_ms(raw_rep.as_dict()) == drop_ms(host_check(one, 1, checks=checks, point_layout=layout)[0])

    # 4. mul_points: one base for K + 1 scalars, then one (scalar, base) record
    ks = m.planted_scalars(msm_pkg.mul_plan(group)["c"], msm_pkg.mul_plan(group)["W"])[0][:17]
    sc, base = m.scalars_bytes(ks, 1), m.base_record(group, layout, m.random_points(group, 1, 17)[0])
    got = cfg.mul_points(sc, base, 17, m.ONE, 1, layout, layout, g2=g2)
    assert got == msm_pkg.host_mul_points(sc, base, 17, m.ONE, 1, layout, layout, g2=g2)
    assert got[16 * stride:] == m.out_record(group, layout, m.expected(group, ks[16], m.random_points(group, 1, 17)[0]))
    got = cfg.mul_points(sc[:32], base, 1, m.EACH, 1, layout, layout, g2=g2)
    assert got == msm_pkg.host_mul_points(sc[:32], base, 1, m.EACH, 1, layout, layout, g2=g2)

    # 5. compress: one non-reduced record among 63
    buf = planted(valid_points(msm_pkg, group, 63), stride, {31: bad[0].encode()})
    out, n_bad = cfg.compress_points(buf, 63, r.PARITY, layout, g2=g2)
    assert (out, n_bad) == msm_pkg.host_compress_points(buf, 63, r.PARITY, layout, g2=g2)
    assert n_bad == 1 and out[31 * r.SIZE[group]:32 * r.SIZE[group]] == b"\xff" * r.SIZE[group]


def test_point_calls_share_one_state_and_leave_the_msm_alone(msm_pkg):
    n = 1 << 10
    points, scalars = msm_pkg.generate_instance_host(o.SEED_BASE + 5, n)
    want = o.decode_jacobian_mont_le(msm_pkg.host_msm(scalars, points, n))
    cfg = msm_pkg.setup_metal_state()
    try:
        assert o.decode_jacobian_mont_le(cfg.msm(scalars, points, n)) == want
        point_calls(cfg, msm_pkg, 1)
        point_calls(cfg, msm_pkg, 2)
        assert o.decode_jacobian_mont_le(cfg.msm(scalars, points, n)) == want
    finally:
        cfg.close()


def test_points_transform_and_fr_calls_share_one_state(msm_pkg):
    """The G1 point calls, the transform and the Fr vector calls use ONE staging set and ONE 64-byte record (counters of a
    check; T and the zero count of an inversion).  On one fresh ctx, in this order, every result equals its host twin: a
    call must see neither the record nor a staged tail of the call before it.  2^12 is a transform of two passes (pass
    buffer and shift powers in use), 2^9 and 2^8 are the tiles of the scan and of the inversion."""
    n = 1 << 10
    points, scalars = msm_pkg.generate_instance_host(o.SEED_BASE + 5, n)
    want = o.decode_jacobian_mont_le(msm_pkg.host_msm(scalars, points, n))
    mont, canon = msm_pkg.SCALAR_MONT_LE, msm_pkg.SCALAR_CANON_LE
    cfg = msm_pkg.setup_metal_state()
    try:
        assert o.decode_jacobian_mont_le(cfg.msm(scalars, points, n)) == want
        big, small = cfg.ntt_domain(t.ARK, 12), cfg.ntt_domain(t.H2C, 9)

        # 1. transform, two passes, with a shift
        data, shift = t.encode(t.random_vector(31, 1 << 12), canon), t.shift_record(9, canon)
        assert cfg.ntt(big, data, t.INVERSE, canon, shift) == msm_pkg.host_ntt(data, t.ARK, 12, t.INVERSE, canon, shift)

        # 2. map of three distinct operands
        a, b, c3 = (f.encode(f.random_values(40 + j, (1 << 9) + 7), mont) for j in range(3))
        k = f.encode([12345], mont)
        assert cfg.fr_map(f.MULSUB_SCALE, a, b, c3, k, mont) == msm_pkg.host_fr_map(f.MULSUB_SCALE, a, b, c3, k, mont)

        # 3. check: the record carries counters
        buf = planted(valid_points(msm_pkg, 1, 257), 64, {256: offenders(1)[1].encode()})
        rep, reasons = cfg.check_points(buf, 257, checks=1, point_layout=c.H2C)
        h_rep, h_reasons = msm_pkg.host_check_points(buf, 257, checks=1, point_layout=c.H2C)
        assert reasons == h_reasons and drop_ms(rep) == drop_ms(h_rep)
        assert rep["n_invalid"] == 1 and rep["first_invalid"] == 256 and reasons.count(0) == 256

        # 4. inversion: the same record carries T and the zero count
        vals = f.random_values(50, (1 << 8) + 1)
        vals[100] = 0
        inv = f.encode(vals, mont)
        got, zeros = cfg.fr_batch_inverse(inv, mont)
        assert (got, zeros) == msm_pkg.host_fr_batch_inverse(inv, mont) and zeros == 1 and got[3200:3232] == bytes(32)

        # 5. mul_points: one base for 17 scalars
        ks = m.planted_scalars(msm_pkg.mul_plan(1)["c"], msm_pkg.mul_plan(1)["W"])[0][:17]
        sc, base = m.scalars_bytes(ks, 1), m.base_record(1, c.H2C, m.random_points(1, 1, 17)[0])
        assert cfg.mul_points(sc, base, 17, m.ONE, 1, c.H2C, c.H2C) == msm_pkg.host_mul_points(sc, base, 17, m.ONE, 1, c.H2C, c.H2C)

        # 6. smaller than what the staging holds by now
        data = t.encode(t.random_vector(32, 1 << 9), mont)
        assert cfg.ntt(small, data, t.FORWARD, mont) == msm_pkg.host_ntt(data, t.H2C, 9, t.FORWARD, mont)
        vecs = f.encode(f.random_values(60, 3 * ((1 << 9) + 1)), canon)
        assert cfg.fr_prefix_product(vecs, f.EXCLUSIVE, canon, 3) == msm_pkg.host_fr_prefix_product(vecs, f.EXCLUSIVE, canon, 3)

        # 7. check again, one valid record: a clean report, and exactly one reason byte written
        one, raw_rep, two_bytes = valid_points(msm_pkg, 1, 1), msm_pkg.CheckReport(), ctypes.create_string_buffer(b"\xAA\xAA", 2)
        assert msm_pkg.lib().msm_amd_check_points(cfg.h, c.H2C, one, 1, 1, two_bytes, ctypes.byref(raw_rep)) == msm_pkg.OK
        assert raw_rep.n_invalid == 0 and raw_rep.first_invalid == 0xFFFFFFFFFFFFFFFF and two_bytes.raw == b"\x00\xAA"
        assert drop_ms(raw_rep.as_dict()) == drop_ms(msm_pkg.host_check_points(one, 1, checks=1, point_layout=c.H2C)[0])

        assert o.decode_jacobian_mont_le(cfg.msm(scalars, points, n)) == want
    finally:
        cfg.close()
