"""CPU-only tests of the pairing calls: the big-integer model against itself and against the golden file, the host twin
(msm_amd_host_pairing_product, msm_amd_host_final_exponentiation) against the model on every layout, the raw Fq12 ops of
the device header run on the host, the planner, the generated constants and the bounds tool.  Every comparison is exact."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import g2_ref as g2
import mul_ref as m
import pairing_ref as pr
from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc")
G1_LAYOUTS, G2_LAYOUTS = m.IN_LAYOUTS[1], m.IN_LAYOUTS[2]


def records(pairs, l1=0, l2=0, z=1):
    return (b"".join(m.base_record(1, l1, p, z) for p, _ in pairs), b"".join(m.base_record(2, l2, q) for _, q in pairs))


def scalar_pairs(rng, n):
    return [(rng.randrange(1, pr.R_ORDER), rng.randrange(1, pr.R_ORDER)) for _ in range(n)]


def points_of(msm_pkg, sp):
    """(a_i G1, b_i G2) as H2C records, by the host twins of the batch multiplication"""
    n = len(sp)
    g1 = msm_pkg.host_mul_points(m.scalars_bytes([a for a, _ in sp], 0), m.base_record(1, 0, o.GEN), n, m.ONE)
    q = msm_pkg.host_mul_points(m.scalars_bytes([b for _, b in sp], 0), m.base_record(2, 0, g2.GEN2), n, m.ONE, g2=True)
    return g1, q


@pytest.fixture(scope="module")
def eight():
    """8 random pairs as model points with their Miller values (shared, not modified)"""
    rng = pr.rng_for(801)
    sp = scalar_pairs(rng, 8)
    pairs = [(pr.g1_mul(a), pr.g2_mul(b)) for a, b in sp]
    return sp, pairs


# ---- the model against itself ------------------------------------------------------------------------------------------
def test_model_is_a_pairing():
    g = pr.pairing(o.GEN, g2.GEN2)
    assert g != pr.ONE12 and pr.pow12(g, pr.R_ORDER) == pr.ONE12
    a, b = 0x1F3, 0x2A7
    assert pr.pairing(pr.g1_mul(a), g2.GEN2) == pr.pow12(g, a)              # linear in the first argument
    assert pr.pairing(o.GEN, pr.g2_mul(b)) == pr.pow12(g, b)                # and in the second
    assert pr.pairing(pr.g1_mul(a), pr.g2_mul(b)) == pr.pow12(g, a * b)
    p1, q = pr.g1_mul(a), pr.g2_mul(b)
    neg_p = (p1[0], (-p1[1]) % pr.P)
    assert pr.mul12(pr.pairing(neg_p, q), pr.pairing(p1, q)) == pr.ONE12
    assert pr.pairing(None, q) == pr.ONE12 and pr.pairing(p1, None) == pr.ONE12


def test_model_final_exponentiation_is_the_plain_power():
    f = pr.miller_loop(pr.g1_mul(3), pr.g2_mul(5))
    assert pr.final_exponentiation(f) == pr.pow12(f, (pr.P**12 - 1) // pr.R_ORDER)
    # the easy part by Frobenius maps agrees with the power: conj = p^6, frob12(., 2) = p^2
    t = pr.mul12(pr.conj12(f), pr.inv12(f))
    assert pr.mul12(pr.frob12(t, 2), t) == pr.pow12(f, (pr.P**6 - 1) * (pr.P**2 + 1))
    assert pr.frob12(f, 1) == pr.pow12(f, pr.P)


def test_golden_file_matches_the_model():
    d = json.load(open(pr.GOLDEN_PATH))
    assert d["pairs"] == pr.golden_entries()
    assert pr.gt_generator() == pr.pairing(o.GEN, g2.GEN2)
    for e in d["pairs"]:
        assert pr.decode_gt(bytes.fromhex(e["gt_mont_le"]), 0) == pr.decode_gt(bytes.fromhex(e["gt_canon_le"]), 1)


def test_dlog_trick_agrees_with_the_model(eight):
    sp, pairs = eight
    assert pr.expected_by_dlog(sp[:2]) == pr.pairing_product(pairs[:2])


# ---- the host twin against the model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", G2_LAYOUTS)
@pytest.mark.parametrize("l1", G1_LAYOUTS)
def test_twin_matches_the_model_on_every_layout(msm_pkg, eight, l1, l2):
    sp, pairs = eight
    a, b = records(pairs, l1, l2, z=0x1234567)
    want = [pr.expected_by_dlog([s]) for s in sp]
    for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
        got, one = msm_pkg.host_pairing_product(a, b, 8, 1, gt_layout=gt, point_layout=l1, g2_point_layout=l2, threads=3)
        assert [pr.decode_gt(got[384 * i:384 * i + 384], gt) for i in range(8)] == want
        assert one == bytes(8)
        assert got == b"".join(pr.encode_gt(w, gt) for w in want)


def test_twin_one_pairing_against_the_models_miller_loop(msm_pkg):
    """not through the discrete-log trick: the twin against the model's own Miller loop and plain power"""
    p1, q = pr.g1_mul(0xABCDEF), pr.g2_mul(0x13579B)
    a, b = records([(p1, q)])
    got, _ = msm_pkg.host_pairing_product(a, b, 1, 1)
    assert pr.decode_gt(got) == pr.pairing(p1, q)


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("group_size", [0, 1, 2, 3, 7])
def test_twin_group_shapes(msm_pkg, n_groups, group_size):
    rng = pr.rng_for(10 * n_groups + group_size)
    sp = scalar_pairs(rng, n_groups * group_size)
    a, b = points_of(msm_pkg, sp) if sp else (b"", b"")
    got, one = msm_pkg.host_pairing_product(a, b, n_groups, group_size, threads=2)
    want = [pr.expected_by_dlog(sp[g * group_size:(g + 1) * group_size]) for g in range(n_groups)]
    assert got == b"".join(pr.encode_gt(w) for w in want)
    assert one == (b"\x01" if group_size == 0 else b"\x00") * n_groups


def test_twin_identities_in_every_slot(msm_pkg, eight):
    sp, pairs = eight
    g = pr.gt_generator()
    for l1, l2 in ((0, 0), (2, 1), (1, 0), (3, 1)):
        # identity in either slot, in both, and in every slot of a group
        cases = [[(None, pairs[0][1])], [(pairs[0][0], None)], [(None, None)], [(None, None)] * 3]
        for case in cases:
            a, b = records(case, l1, l2)
            got, one = msm_pkg.host_pairing_product(a, b, 1, len(case), point_layout=l1, g2_point_layout=l2)
            assert got == pr.encode_gt(pr.ONE12) and one == b"\x01"
        for slot in range(3):                      # an identity at each place of a group of three
            case = [pairs[i] for i in range(3)]
            case[slot] = (None, case[slot][1]) if slot % 2 else (case[slot][0], None)
            a, b = records(case, l1, l2)
            got, one = msm_pkg.host_pairing_product(a, b, 1, 3, point_layout=l1, g2_point_layout=l2)
            left = [sp[i] for i in range(3) if i != slot]
            assert pr.decode_gt(got) == pr.expected_by_dlog(left) and one == b"\x00"
    assert g != pr.ONE12


def test_twin_is_one_on_cancelling_groups(msm_pkg):
    a = 0x55AA55
    q = pr.g2_mul(77)
    p1 = pr.g1_mul(a)
    neg = (p1[0], (-p1[1]) % pr.P)
    ra, rb = records([(p1, q), (neg, q), (p1, q), (pr.g1_mul(pr.R_ORDER - a - 1), q)])
    got, one = msm_pkg.host_pairing_product(ra, rb, 2, 2)
    assert one == b"\x01\x00"                        # the second group is off by one G1
    assert got[:384] == pr.encode_gt(pr.ONE12)
    assert pr.decode_gt(got[384:]) == pr.pow12(pr.pairing(o.GEN, q), pr.R_ORDER - 1)


def test_twin_larger_group_by_the_dlog_trick(msm_pkg):
    rng = pr.rng_for(130)
    sp = scalar_pairs(rng, 130)
    a, b = points_of(msm_pkg, sp)
    got, one = msm_pkg.host_pairing_product(a, b, 1, 130)
    assert pr.decode_gt(got) == pr.expected_by_dlog(sp) and one == b"\x00"
    got2, _ = msm_pkg.host_pairing_product(a, b, 1, 130, threads=1)
    assert got2 == got


def test_twin_miller_only_and_final_exponentiation(msm_pkg, eight):
    sp, pairs = eight
    a, b = records(pairs)
    want, _ = msm_pkg.host_pairing_product(a, b, 4, 2)
    for gt in (pr.GT_MONT_LE, pr.GT_CANON_LE):
        mil, none = msm_pkg.host_pairing_product(a, b, 4, 2, flags=pr.PAIRING_MILLER_ONLY, gt_layout=gt)
        assert none is None
        for g in range(4):
            f = pr.decode_gt(mil[384 * g:384 * g + 384], gt)
            if g == 0:                            # the model's plain power (0.2 s) once, the x-power chain for the rest
                assert pr.final_exponentiation(f) == pr.expected_by_dlog(sp[:2])
        fin, one = msm_pkg.host_final_exponentiation(mil, 4, gt)
        assert [pr.decode_gt(fin[384 * g:384 * g + 384], gt) for g in range(4)] == \
               [pr.decode_gt(want[384 * g:384 * g + 384]) for g in range(4)]
        assert one == bytes(4)
    fin, one = msm_pkg.host_final_exponentiation(pr.encode_gt(pr.ONE12), 1)
    assert fin == pr.encode_gt(pr.ONE12) and one == b"\x01"


def test_twin_argument_errors_leave_the_output_untouched(msm_pkg, eight):
    _, pairs = eight
    a, b = records(pairs[:2])
    L = msm_pkg.lib()
    out = ctypes.create_string_buffer(b"\xA5" * 768, 768)
    flag = ctypes.create_string_buffer(b"\xA5" * 2, 2)
    bad = [
        (0, 0, a, b, 2, 1, 2, 0, out, None, 1),                    # unknown flag
        (0, 0, a, b, 2, 1, 1, 0, out, flag, 1),                    # is_one with MILLER_ONLY
        (0, 0, a, b, 2, 1, 0, 2, out, flag, 1),                    # unknown GT layout
        (4, 0, a, b, 2, 1, 0, 0, out, flag, 1),                    # PREPARED is a device layout
        (5, 0, a, b, 2, 1, 0, 0, out, flag, 1),                    # table handles
        (0, 2, a, b, 2, 1, 0, 0, out, flag, 1),
        (0, 3, a, b, 2, 1, 0, 0, out, flag, 1),
        (0, 0, None, b, 2, 1, 0, 0, out, flag, 1),                 # null with work to do
        (0, 0, a, None, 2, 1, 0, 0, out, flag, 1),
        (0, 0, a, b, 2, 1, 0, 0, None, flag, 1),
        (0, 0, a, b, 1 << 16, 1 << 16, 0, 0, out, flag, 1),        # 2^32 pairs
        (0, 0, a, b, 1 << 33, 0, 0, 0, out, flag, 1),
    ]
    for args in bad:
        assert L.msm_amd_host_pairing_product(*args) == msm_pkg.INPUT_ERROR, args
        assert out.raw == b"\xA5" * 768 and flag.raw == b"\xA5" * 2
    assert L.msm_amd_host_pairing_product(0, 0, None, None, 0, 5, 0, 0, None, None, 1) == msm_pkg.OK     # n_groups = 0
    assert L.msm_amd_host_final_exponentiation(2, a, 1, out, None, 1) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_final_exponentiation(0, None, 1, out, None, 1) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_host_final_exponentiation(0, None, 0, None, None, 1) == msm_pkg.OK
    assert out.raw == b"\xA5" * 768


# ---- the raw ops of the device header, run on the host --------------------------------------------------------------------
def raw_cases(rng):
    """(op, a words, b words, check(out words)) with operands at the contract's edge: every component at 4 p - 1 p
    steps (fe_rec puts half of them at the maximum multiple) and limbs that borrow from their neighbours"""
    a, b = pr.rand_fq12(rng), pr.rand_fq12(rng)
    cyc = pr.rand_cyclotomic(rng)
    A = lambda x: pr.fq12_rec(x, 4, rng)
    yield "mul", pr.FQ12_OP_MUL, A(a), A(b), lambda w: pr.fq12_of(w) == pr.mul12(a, b)
    yield "sqr", pr.FQ12_OP_SQR, A(a), [], lambda w: pr.fq12_of(w) == pr.sqr12(a)
    yield "cyclo", pr.FQ12_OP_CYCLO_SQR, A(cyc), [], lambda w: pr.fq12_of(w) == pr.sqr12(cyc)
    for k, op in ((1, pr.FQ12_OP_FROB1), (2, pr.FQ12_OP_FROB2), (3, pr.FQ12_OP_FROB3)):
        yield "frob%d" % k, op, A(a), [], lambda w, k=k: pr.fq12_of(w) == pr.frob12(a, k)
    yield "conj", pr.FQ12_OP_CONJ, A(a), [], lambda w: pr.fq12_of(w) == pr.conj12(a)
    yield "inv", pr.FQ12_OP_INV, A(a), [], lambda w: pr.fq12_of(w) == pr.inv12(a)
    yield "pow_x", pr.FQ12_OP_POW_X, A(cyc), [], lambda w: pr.fq12_of(w) == pr.pow12(cyc, pr.X_BN)
    # Fq6: the even powers of w
    a6, b6 = (a[0], pr.ZERO2, a[2], pr.ZERO2, a[4], pr.ZERO2), (b[0], pr.ZERO2, b[2], pr.ZERO2, b[4], pr.ZERO2)
    want6 = pr.mul12(a6, b6)
    yield "fq6", pr.FQ12_OP_FQ6_MUL, A(a6)[:54], A(b6)[:54], \
        lambda w: [g2.fq2_of(w[18 * k:18 * k + 18]) for k in range(3)] == [want6[0], want6[2], want6[4]] and \
        not any(w[54:])
    l = [g2.rand_fq2(rng) for _ in range(3)]
    lw = sum((g2.fq2_rec(c, 8, rng) for c in l), [])
    yield "line", pr.FQ12_OP_LINE_MUL, A(a), lw, lambda w: pr.fq12_of(w) == pr.mul12(a, pr.line12(*l))
    # the steps: T a random projective form of a point, Q another point, P a G1 point (canonical limbs)
    t_aff, q_aff, p1 = pr.g2_mul(rng.randrange(1, pr.R_ORDER)), pr.g2_mul(rng.randrange(1, pr.R_ORDER)), pr.g1_mul(777)
    z = g2.rand_fq2(rng)
    T = (pr.mul2(t_aff[0], z), pr.mul2(t_aff[1], z), z)
    tw = sum((g2.fq2_rec(c, 4, rng) for c in T), [])
    pw = g2.limbs_of(p1[0] * pr.RHO % pr.P) + g2.limbs_of(p1[1] * pr.RHO % pr.P)

    def step_ok(w, want):
        (T3, line) = want
        got_t = tuple(g2.fq2_of(w[18 * k:18 * k + 18]) for k in range(3))
        got_l = tuple(g2.fq2_of(w[54 + 18 * k:72 + 18 * k]) for k in range(3))
        return got_t == T3 and got_l == line

    yield "double", pr.FQ12_OP_DOUBLE_STEP, tw, pw, lambda w: step_ok(w, pr.double_step(T, p1))
    for negated in (False, True):                   # Q.y canonical, or a negation at 4 p - y
        qw, qq = g2.aff_rec(q_aff, rng, negated)
        yield "add", pr.FQ12_OP_ADD_STEP, tw + qw, pw, lambda w, qq=qq: step_ok(w, pr.add_step(T, qq, p1))
    # T = Q: zeros throughout.  T = -Q: the point at infinity (0, Y', 0) and the vertical line (0, l1, l3), as the
    # polynomial map gives them.  No fault either way (division-free)
    t1 = (q_aff[0], q_aff[1], pr.ONE2)
    t1w = sum((g2.fq2_rec(c, 1, rng) for c in t1), [])
    qw, _ = g2.aff_rec(q_aff, rng)
    yield "add T=Q", pr.FQ12_OP_ADD_STEP, t1w + qw, pw, \
        lambda w: all(g2.fq2_of(w[18 * k:18 * k + 18]) == pr.ZERO2 for k in range(6))
    t2 = (q_aff[0], pr.neg2(q_aff[1]), pr.ONE2)
    t2w = sum((g2.fq2_rec(c, 4, rng) for c in t2), [])
    want2 = pr.add_step(t2, q_aff, p1)
    assert want2[0][0] == want2[0][2] == want2[1][0] == pr.ZERO2 and pr.ZERO2 not in (want2[0][1], want2[1][1], want2[1][2])
    yield "add T=-Q", pr.FQ12_OP_ADD_STEP, t2w + qw, pw, lambda w: step_ok(w, want2)


def check_raw_outputs(name, w):
    """every output is an element of the contract: normalised limbs, at most 4 p per component (line l3: 8 p)"""
    comps = [g2.value(w[9 * i:9 * i + 9]) for i in range(12)]
    assert g2.normalised(w, 12), name
    assert all(v <= 8 * pr.P for v in comps), name
    if name not in ("double", "add", "add T=Q", "add T=-Q"):
        assert all(v <= 4 * pr.P for v in comps), name


def test_raw_ops_on_the_host_match_the_limb_model(msm_pkg):
    for seed in (1, 2):
        for name, op, a, b, ok in raw_cases(pr.rng_for(4000 + seed)):
            w = msm_pkg.test_fq12_op_host(op, a, b)
            assert ok(w), name
            check_raw_outputs(name, w)
    assert msm_pkg.lib().msm_amd_test_fq12_op_host(14, (ctypes.c_uint32 * 108)(), (ctypes.c_uint32 * 108)(),
                                                   (ctypes.c_uint32 * 108)()) == msm_pkg.INPUT_ERROR
    assert msm_pkg.lib().msm_amd_test_fq12_op_host(-1, (ctypes.c_uint32 * 108)(), (ctypes.c_uint32 * 108)(),
                                                   (ctypes.c_uint32 * 108)()) == msm_pkg.INPUT_ERROR


# ---- the planner --------------------------------------------------------------------------------------------------------
def test_planner_grid(msm_pkg):
    for n_groups in (1, 2, 3, 65, 255, 256, 257, 1 << 14):
        for group_size in (0, 1, 2, 3, 4, 5, 63, 64, 65, 130, 1 << 10):
            for knob in (0, 1, 2, 4, 3, 9):
                for final_from in (0, 256, 1 << 40):
                    p = msm_pkg.pairing_plan(n_groups, group_size, knob, final_from)
                    ppl, lpg = p["pairs_per_lane"], p["lanes_per_group"]
                    assert ppl in (1, 2, 4)
                    if knob in (1, 2, 4):
                        assert ppl == knob
                    elif knob:
                        assert ppl == 1                                 # pairs_per_lane = 1 is always valid
                    # the lanes of a group cover its pairs exactly once: lane l takes l ppl .. min((l + 1) ppl, size)
                    covered = [i for l in range(lpg) for i in range(l * ppl, min((l + 1) * ppl, group_size))]
                    assert covered == list(range(group_size))
                    assert lpg == max(1, -(-group_size // ppl))
                    levels, c = 0, lpg
                    while c > 1:
                        c, levels = -(-c // 4), levels + 1
                    assert p["fold_levels"] == levels
                    assert p["final_on_device"] == (1 if n_groups >= final_from else 0)
    big = msm_pkg.pairing_plan(1, 1 << 18)                  # one pair per lane at every size until larger ones are timed
    assert big["pairs_per_lane"] == 1 and big["lanes_per_group"] == 1 << 18 and big["fold_levels"] == 9
    # the library's own threshold (device_final_from left out): the measured crossover, 768
    assert [msm_pkg.pairing_plan(n, 1)["final_on_device"] for n in (1, 767, 768, 1 << 14)] == [0, 0, 1, 1]
    assert msm_pkg.pairing_plan(1 << 14, 1)["pairs_per_lane"] == 1
    out = (ctypes.c_uint32 * 4)()
    assert msm_pkg.lib().msm_amd_test_pairing_plan(1 << 16, 1 << 16, 0, 0, out) == msm_pkg.INPUT_ERROR


# ---- constants, bounds, exports -----------------------------------------------------------------------------------------
def test_generated_constants_match_the_headers():
    tool = os.path.join(ROOT, "tools", "gen_fq12_constants.py")
    for which, name in (("device", "bn254_fq12_29_consts.inc"), ("host", "host_fq12_64_consts.inc")):
        out = subprocess.run([sys.executable, tool, which], check=True, capture_output=True, text=True).stdout
        assert out == open(os.path.join(CSRC, name)).read(), name
    masks = "0xA1818041C0864428ull, kAteNeg = 0x0408100802100880ull"
    assert masks in open(os.path.join(CSRC, "bn254_fq12_29.hip.h")).read()
    assert masks.replace("kAte", "kHostAte") in open(os.path.join(CSRC, "host_fq12_64.h")).read()
    # and they are the model's: gamma, 3 b', the digits
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_fq12_constants as gen
    assert gen.GAMMA == pr.GAMMA and gen.B3 == pr.B3 and gen.ATE == pr.ATE


def test_bounds_tool_agrees_with_the_header():
    tool = os.path.join(ROOT, "tools", "fq12_bounds.py")
    out = subprocess.run([sys.executable, tool, "--check-header"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all figures of bn254_fq12_29.hip.h re-derived" in out.stdout


def test_exports_constants_and_bindings(msm_pkg):
    L = msm_pkg.lib()
    for name in ("msm_amd_pairing_product", "msm_amd_pairing_product_device", "msm_amd_host_pairing_product",
                 "msm_amd_final_exponentiation", "msm_amd_final_exponentiation_device",
                 "msm_amd_host_final_exponentiation", "msm_amd_test_pairing_plan", "msm_amd_test_fq12_op",
                 "msm_amd_test_fq12_op_host", "msm_amd_test_fq12_ops", "msm_amd_test_fq12_ops_host"):
        assert name in msm_pkg.EXPORTS and hasattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "msm_amd.h")).read()
    for text in ("MSM_AMD_GT_MONT_LE = 0", "MSM_AMD_GT_CANON_LE = 1", "MSM_AMD_GT_BYTES = 384",
                 "MSM_AMD_PAIRING_MILLER_ONLY = 1", "MSM_AMD_FQ12_OP_ADD_STEP = 12", "MSM_AMD_FQ12_OP_FINAL_EXP = 13",
                 "MSM_AMD_FQ12_WORDS = 108"):
        assert text in hdr
    assert (msm_pkg.GT_MONT_LE, msm_pkg.GT_CANON_LE, msm_pkg.GT_BYTES, msm_pkg.PAIRING_MILLER_ONLY) == (0, 1, 384, 1)
    assert msm_pkg.FQ12_OP_ADD_STEP == 12 == pr.FQ12_OP_ADD_STEP and msm_pkg.FQ12_WORDS == 108
    assert msm_pkg.FQ12_OP_FINAL_EXP == 13 == pr.FQ12_OP_FINAL_EXP
    for f in ("pairing_product", "pairing_product_device", "final_exponentiation", "final_exponentiation_device",
              "test_fq12_op", "test_fq12_ops"):
        assert hasattr(msm_pkg.MsmConfig, f)
