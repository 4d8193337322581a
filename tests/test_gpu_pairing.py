"""GPU tests of the pairing calls: the raw Fq12 ops against the limb model, pairing products against the big-integer
model and the host twin over every layout, plan boundary, identity placement and flag.  Every comparison is exact.
Larger groups use the discrete-log trick (pairs (a_i G1, b_i G2) multiply to g^(sum a_i b_i)); calls with many groups are
compared with the host twin on every group and with the model on the first, the middle and the last one."""
import ctypes

import pytest

import check_ref as c
import g2_ref as g2
import mul_ref as m
import pairing_ref as pr
from oracle import bn254_ref as o
from test_pairing_host import check_raw_outputs, points_of, raw_cases, records, scalar_pairs

pytestmark = pytest.mark.gpu
GT = pr.GT_BYTES
POOL = 400


@pytest.fixture(scope="module")
def pool(msm_pkg):
    """400 pairs (a_i G1, b_i G2) as H2C records with their scalars (shared, not modified)"""
    sp = scalar_pairs(pr.rng_for(9001), POOL)
    a, b = points_of(msm_pkg, sp)
    return sp, a, b


@pytest.fixture(scope="module")
def eight():
    sp = scalar_pairs(pr.rng_for(801), 8)
    return sp, [(pr.g1_mul(a), pr.g2_mul(b)) for a, b in sp]


def knobs(monkeypatch, ppl=None, final_from=None, lds=None):
    for name, v in (("MSM_AMD_PAIRING_PAIRS_PER_LANE", ppl), ("MSM_AMD_PAIRING_DEVICE_FINAL_FROM", final_from),
                    ("MSM_AMD_PAIRING_F_IN_LDS", lds)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def on_device(cfg, data):
    d = cfg.alloc(max(1, len(data)))
    if data:
        cfg.to_device(d, data)
    return d


def groups_of(buf, n):
    return [buf[GT * i:GT * i + GT] for i in range(n)]


# ---- 1. raw ops ----------------------------------------------------------------------------------------------------------
def test_raw_ops_match_the_limb_model_and_the_host(cfg, msm_pkg):
    for name, op, a, b, ok in raw_cases(pr.rng_for(4001)):
        w = cfg.test_fq12_op(op, a, b)
        assert ok(w), name
        check_raw_outputs(name, w)
        assert w == msm_pkg.test_fq12_op_host(op, a, b), name          # bit for bit, limbs included
    z = (ctypes.c_uint32 * 108)()
    assert msm_pkg.lib().msm_amd_test_fq12_op(cfg.h, 14, z, z, z) == msm_pkg.INPUT_ERROR
    assert msm_pkg.lib().msm_amd_test_fq12_op(cfg.h, -1, z, z, z) == msm_pkg.INPUT_ERROR


# ---- 2. every layout against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", m.IN_LAYOUTS[2])
@pytest.mark.parametrize("l1", m.IN_LAYOUTS[1])
def test_product_matches_the_model_on_every_layout(cfg, monkeypatch, eight, l1, l2):
    sp, pairs = eight
    a, b = records(pairs, l1, l2, z=0x7654321)
    want = [pr.expected_by_dlog([s]) for s in sp]
    knobs(monkeypatch, final_from=0)
    for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
        got, one = cfg.pairing_product(a, b, 8, 1, gt_layout=gt, point_layout=l1, g2_point_layout=l2)
        assert got == b"".join(pr.encode_gt(w, gt) for w in want) and one == bytes(8)
    got, one = cfg.pairing_product(a, b, 2, 4, point_layout=l1, g2_point_layout=l2)
    assert got == b"".join(pr.encode_gt(pr.expected_by_dlog(sp[4 * g:4 * g + 4])) for g in range(2)) and one == bytes(2)


def test_one_pairing_against_the_models_miller_loop(cfg, monkeypatch):
    p1, q = pr.g1_mul(0xABCDEF), pr.g2_mul(0x13579B)
    a, b = records([(p1, q)])
    knobs(monkeypatch, final_from=0)
    got, _ = cfg.pairing_product(a, b, 1, 1)
    assert pr.decode_gt(got) == pr.pairing(p1, q)


def test_device_forms_with_host_layouts_and_prepared_records(cfg, msm_pkg, eight):
    sp, pairs = eight
    want = b"".join(pr.encode_gt(pr.expected_by_dlog(sp[2 * g:2 * g + 2])) for g in range(4))
    bufs = []
    try:
        d_out, d_one = cfg.alloc(4 * GT), cfg.alloc(4)
        bufs += [d_out, d_one]
        for l1, l2 in ((c.H2C, c.G2_H2C), (c.ARK_PROJECTIVE, c.G2_ARK), (c.JAC_BE32, c.G2_H2C), (c.ARK_AFFINE, c.G2_ARK)):
            a, b = records(pairs, l1, l2, z=99)
            d_a, d_b = on_device(cfg, a), on_device(cfg, b)
            bufs += [d_a, d_b]
            cfg.to_device(d_out, b"\xA5" * (4 * GT))
            ms = cfg.pairing_product_device(d_a, d_b, 4, 2, d_out, d_one, point_layout=l1, g2_point_layout=l2)
            assert cfg.to_host(d_out, 4 * GT) == want and cfg.to_host(d_one, 4) == bytes(4) and ms > 0
        # PREPARED records of both groups, made on the device from the affine ones
        a, b = records(pairs)
        d_a, d_b = on_device(cfg, a), on_device(cfg, b)
        d_pa, d_pb = cfg.bases_prepare_device(d_a, 8), cfg.g2_bases_prepare_device(d_b, 8)
        bufs += [d_a, d_b, d_pa, d_pb]
        cfg.pairing_product_device(d_pa, d_pb, 4, 2, d_out, None, point_layout=msm_pkg.POINT_PREPARED,
                                   g2_point_layout=msm_pkg.G2_POINT_PREPARED)
        assert cfg.to_host(d_out, 4 * GT) == want
        cfg.pairing_product_device(d_pa, d_b, 4, 2, d_out, None, point_layout=msm_pkg.POINT_PREPARED)
        assert cfg.to_host(d_out, 4 * GT) == want
    finally:
        for d in bufs:
            cfg.free(d)


# ---- 3. every boundary of the plan ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("n_groups", [1, 3, 65])
@pytest.mark.parametrize("ppl", [1, 2, 4])
def test_shapes_across_the_plan(cfg, msm_pkg, monkeypatch, pool, ppl, n_groups, lds):
    sp, a, b = pool
    for group_size in (1, 2, 3, 63, 64, 65, 130):
        n = n_groups * group_size
        if n > POOL:
            continue
        plan = msm_pkg.pairing_plan(n_groups, group_size, ppl, 0)
        assert plan["pairs_per_lane"] == ppl and plan["lanes_per_group"] == -(-group_size // ppl)
        twin, twin_one = msm_pkg.host_pairing_product(a[:64 * n], b[:128 * n], n_groups, group_size)
        for g in sorted({0, n_groups // 2, n_groups - 1}):
            assert pr.decode_gt(twin[GT * g:GT * g + GT]) == pr.expected_by_dlog(sp[g * group_size:(g + 1) * group_size])
        for final_from in (0, 1 << 40):                 # the final exponentiation on the device, then on the host
            knobs(monkeypatch, ppl, final_from, lds)          # lds: the running f in private memory or in LDS
            got, one = cfg.pairing_product(a[:64 * n], b[:128 * n], n_groups, group_size)
            assert got == twin and one == twin_one == bytes(n_groups), (group_size, final_from)


def test_default_plan_and_group_size_zero(cfg, monkeypatch, pool):
    sp, a, b = pool
    knobs(monkeypatch)
    got, one = cfg.pairing_product(a[:64 * 6], b[:128 * 6], 2, 3)
    assert got == b"".join(pr.encode_gt(pr.expected_by_dlog(sp[3 * g:3 * g + 3])) for g in range(2)) and one == bytes(2)
    for final_from in (0, 1 << 40):
        knobs(monkeypatch, final_from=final_from)
        got, one = cfg.pairing_product(None, None, 3, 0)
        assert got == pr.encode_gt(pr.ONE12) * 3 and one == b"\x01" * 3
    assert cfg.pairing_product(a, b, 0, 5) == (b"", b"")


# ---- 4. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppl", [1, 2, 4])
def test_identities_at_the_edges_of_a_lane(cfg, msm_pkg, monkeypatch, eight, ppl):
    sp, pairs = eight
    ident = {0: (None, pairs[0][1]), 1: (pairs[1][0], None), 2: (None, None)}
    cases = []
    for holes in ([0], [ppl - 1], [7], [0, 7], list(range(ppl)), list(range(8 - ppl, 8)), list(range(8))):
        case = list(pairs)
        for k, i in enumerate(holes):
            case[i] = ident[k % 3]
        cases.append((case, [s for i, s in enumerate(sp) if i not in holes]))
    for l1, l2 in ((c.H2C, c.G2_H2C), (c.ARK_AFFINE, c.G2_ARK), (c.ARK_PROJECTIVE, c.G2_H2C)):
        for case, left in cases:
            a, b = records(case, l1, l2)
            want = pr.expected_by_dlog(left) if left else pr.ONE12
            for final_from, lds in ((0, 0), (1 << 40, 1)):
                knobs(monkeypatch, ppl, final_from, lds)
                got, one = cfg.pairing_product(a, b, 1, 8, point_layout=l1, g2_point_layout=l2)
                assert got == pr.encode_gt(want) and one == (b"\x00" if left else b"\x01")
            if l1 == c.H2C:
                assert msm_pkg.host_pairing_product(a, b, 1, 8)[0] == pr.encode_gt(want)


# ---- 5. the pairing check ---------------------------------------------------------------------------------------------------------
def test_is_one_on_cancelling_groups_and_off_by_one(cfg, monkeypatch):
    a = 0x55AA55
    q, q2 = pr.g2_mul(77), pr.g2_mul(78)
    p1 = pr.g1_mul(a)
    neg = (p1[0], (-p1[1]) % pr.P)
    ra, rb = records([(p1, q), (neg, q), (p1, q), (pr.g1_mul(pr.R_ORDER - a - 1), q), (p1, q), (neg, q2),
                      (pr.g1_mul(3), pr.g2_mul(5)), (pr.g1_mul(pr.R_ORDER - 5), pr.g2_mul(3))])
    for final_from in (0, 1 << 40):
        knobs(monkeypatch, final_from=final_from)
        got, one = cfg.pairing_product(ra, rb, 4, 2, gt_layout=pr.GT_CANON_LE)
        assert one == b"\x01\x00\x00\x01"
        assert got[:GT] == pr.encode_gt(pr.ONE12, pr.GT_CANON_LE) == got[3 * GT:]
        assert pr.decode_gt(got[GT:2 * GT], 1) == pr.gt_pow(pr.gt_generator(), -77)
        assert pr.decode_gt(got[2 * GT:3 * GT], 1) == pr.gt_pow(pr.gt_generator(), -a)


# ---- 6, 7. the stage tap, host and device forms, the twin ---------------------------------------------------------------------------
def test_miller_only_then_final_exponentiation_equals_one_call(cfg, msm_pkg, monkeypatch, pool):
    sp, a, b = pool
    n_groups, size = 5, 9
    n = n_groups * size
    a, b = a[:64 * n], b[:128 * n]
    knobs(monkeypatch, 2, 0)
    want, want_one = cfg.pairing_product(a, b, n_groups, size)
    twin, _ = msm_pkg.host_pairing_product(a, b, n_groups, size)
    assert want == twin
    assert pr.decode_gt(want[:GT]) == pr.expected_by_dlog(sp[:size])
    d_a, d_b, d_mil, d_out, d_one = on_device(cfg, a), on_device(cfg, b), cfg.alloc(n_groups * GT), cfg.alloc(n_groups * GT), cfg.alloc(n_groups)
    try:
        for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
            mil, none = cfg.pairing_product(a, b, n_groups, size, flags=pr.PAIRING_MILLER_ONLY, gt_layout=gt)
            assert none is None
            knobs(monkeypatch, 2, 0, 1)                                                       # the same Miller bytes from LDS
            assert cfg.pairing_product(a, b, n_groups, size, flags=pr.PAIRING_MILLER_ONLY, gt_layout=gt)[0] == mil
            knobs(monkeypatch, 2, 0)
            # the Miller product is a representative; the device and the twin write the same one
            assert mil == msm_pkg.host_pairing_product(a, b, n_groups, size, flags=pr.PAIRING_MILLER_ONLY, gt_layout=gt)[0]
            cfg.pairing_product_device(d_a, d_b, n_groups, size, d_mil, None, flags=pr.PAIRING_MILLER_ONLY, gt_layout=gt)
            assert cfg.to_host(d_mil, n_groups * GT) == mil
            ms = cfg.final_exponentiation_device(d_mil, n_groups, d_out, d_one, gt_layout=gt)
            fin = cfg.to_host(d_out, n_groups * GT)
            assert [pr.decode_gt(r, gt) for r in groups_of(fin, n_groups)] == [pr.decode_gt(r) for r in groups_of(want, n_groups)]
            assert cfg.to_host(d_one, n_groups) == want_one and ms > 0
            cfg.final_exponentiation_device(d_mil, n_groups, d_mil, None, gt_layout=gt)       # in place
            assert cfg.to_host(d_mil, n_groups * GT) == fin
            for final_from in (0, 1 << 40):                                                   # host buffers, both placements
                knobs(monkeypatch, 2, final_from)
                assert cfg.final_exponentiation(mil, n_groups, gt) == (fin, want_one)
            assert msm_pkg.host_final_exponentiation(mil, n_groups, gt) == (fin, want_one)
        # the device form of the whole call
        cfg.pairing_product_device(d_a, d_b, n_groups, size, d_out, d_one)
        assert cfg.to_host(d_out, n_groups * GT) == want and cfg.to_host(d_one, n_groups) == want_one
    finally:
        for d in (d_a, d_b, d_mil, d_out, d_one):
            cfg.free(d)


def test_argument_errors_leave_the_output_untouched(cfg, msm_pkg, eight):
    _, pairs = eight
    a, b = records(pairs[:2])
    L = msm_pkg.lib()
    out = ctypes.create_string_buffer(b"\xA5" * 768, 768)
    flag = ctypes.create_string_buffer(b"\xA5" * 2, 2)
    bad = [(0, 0, a, b, 2, 1, 2, 0, out, None), (0, 0, a, b, 2, 1, 1, 0, out, flag), (0, 0, a, b, 2, 1, 0, 2, out, flag),
           (4, 0, a, b, 2, 1, 0, 0, out, flag), (5, 0, a, b, 2, 1, 0, 0, out, flag), (0, 2, a, b, 2, 1, 0, 0, out, flag),
           (0, 3, a, b, 2, 1, 0, 0, out, flag), (0, 0, None, b, 2, 1, 0, 0, out, flag), (0, 0, a, None, 2, 1, 0, 0, out, flag),
           (0, 0, a, b, 2, 1, 0, 0, None, flag), (0, 0, a, b, 1 << 16, 1 << 16, 0, 0, out, flag)]
    for args in bad:
        assert L.msm_amd_pairing_product(cfg.h, *args) == msm_pkg.INPUT_ERROR, args
        assert out.raw == b"\xA5" * 768 and flag.raw == b"\xA5" * 2
    ms = ctypes.c_float(0)
    # table handles in the device form
    assert L.msm_amd_pairing_product_device(cfg.h, 5, 0, a, b, 2, 1, 0, 0, out, None, ctypes.byref(ms)) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_pairing_product_device(cfg.h, 0, 3, a, b, 2, 1, 0, 0, out, None, ctypes.byref(ms)) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_final_exponentiation(cfg.h, 2, a, 1, out, None) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_final_exponentiation(cfg.h, 0, None, 1, out, None) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_final_exponentiation(cfg.h, 0, None, 0, None, None) == msm_pkg.OK
    assert out.raw == b"\xA5" * 768
    assert L.msm_amd_pairing_product(cfg.h, 0, 0, None, None, 0, 7, 0, 0, None, None) == msm_pkg.OK


# ---- 8, 9. the ctx afterwards; invalid points -----------------------------------------------------------------------------------------
def test_ctx_runs_an_msm_afterwards(cfg, msm_pkg, monkeypatch, pool):
    sp, a, b = pool
    knobs(monkeypatch, final_from=0)
    got, _ = cfg.pairing_product(a[:64 * 4], b[:128 * 4], 1, 4)
    assert pr.decode_gt(got) == pr.expected_by_dlog(sp[:4])
    ks = [3, 5, 7, 11]
    out = cfg.msm(m.scalars_bytes(ks, 0), a[:64 * 4], 4)
    want = pr.g1_mul(sum(k * s for k, (s, _) in zip(ks, sp[:4])) % pr.R_ORDER)
    assert o.decode_jacobian_mont_le(out) == want


def test_invalid_points_return_and_the_next_call_is_right(cfg, msm_pkg, monkeypatch, eight):
    """points off the curve and outside the r-torsion: the result is unspecified, the call returns OK (the formulas are
    division-free: nothing is provoked) and the next valid call is correct"""
    sp, pairs = eight
    off1 = (pairs[0][0][0], (pairs[0][0][1] + 1) % pr.P)                 # not on the curve
    off2 = (pairs[0][1][0], ((pairs[0][1][1][0] + 1) % pr.P, pairs[0][1][1][1]))
    small = m.small_order_point()                                        # on the twist, order 10069: outside the r-torsion
    rng = pr.rng_for(5)
    junk1, junk2 = (rng.randrange(pr.P), rng.randrange(pr.P)), (g2.rand_fq2(rng), g2.rand_fq2(rng))
    bad = [(off1, pairs[0][1]), (pairs[1][0], off2), (pairs[2][0], small), (junk1, junk2), (pairs[3][0], small),
           (off1, off2), (junk1, pairs[1][1]), (pairs[1][0], junk2)]
    a, b = records(bad)
    a_ok, b_ok = records(pairs)
    want = b"".join(pr.encode_gt(pr.expected_by_dlog(sp[4 * g:4 * g + 4])) for g in range(2))
    for ppl in (1, 4):
        for final_from in (0, 1 << 40):
            knobs(monkeypatch, ppl, final_from)
            got, one = cfg.pairing_product(a, b, 2, 4)
            assert len(got) == 2 * GT and len(one) == 2
            assert all(int.from_bytes(got[32 * i:32 * i + 32], "little") < pr.P for i in range(24))   # still canonical
            assert cfg.pairing_product(a_ok, b_ok, 2, 4) == (want, bytes(2))
