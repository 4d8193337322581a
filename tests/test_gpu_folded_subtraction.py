"""Whole MSMs through the point additions whose lifted subtractions ride on the Montgomery reductions (Fq29::mul_sub_np /
sqr_sub_np), bit-exact against the oracle's canonical affine result.

n = 2^10 and 2^12 with the window forced to c = 5, 13, 16 and 17: the smallest shapes that reach phase A (affine start)
and phase B (mixed additions) of accumulate_kernel, split buckets with the combine kernels, and both sum_groups levels
with reduce_bits.  Two instances per size -- random scalars with the exceptional buckets planted among them (identity
bases, one base repeated in a bucket: the doubling with its re-gather, P and -P in a bucket: the vanishing sum), and
all scalars equal (one long bucket per window, cut at CH) -- each through both record kinds: the caller's records
gathered in place (ExtBases, the instance on E') and the packed copy of msm_amd_bases_prepare_device (PackedBases).
The raw ops of the folded forms run on the device against their host twin as well."""
import random

import pytest

import test_folded_subtraction_host as host
from oracle import bn254_ref as o
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
R = o.R_ORDER
SIZES = (1 << 10, 1 << 12)
WINDOWS = (5, 13, 16, 17)


def decode(out96):
    return o.decode_jacobian_mont_le(out96)


def planted(n, seed):
    """(scalars, points) bytes: a generated instance with, from record 8 on, buckets that every window shares (one
    scalar each): Z P Z (identities around a base), P P (affine start meets its own base: doubling), P P 2P 4P 8P
    (doublings inside the mixed addition: the base is gathered again), the same under the scalar r - k (every digit
    negative), P -P (vanishes), P -P Q Q (vanishes, restarts, doubles)"""
    pts, sc = co.gen_instance(o.SEED_BASE + 9100 + seed, n)
    pts, sc = bytearray(pts), bytearray(sc)
    rng = random.Random(seed)
    P = o.scalar_mul(rng.randrange(1, R), o.GEN)
    Q = o.scalar_mul(rng.randrange(1, R), o.GEN)
    chain = [P, P] + [o.scalar_mul(2 ** j, P) for j in (1, 2, 3)]
    groups = [([None, P, None], 5), ([P, P], 7), (chain, (1 << 14) + 1), (chain, R - (1 << 33) - 7),
              ([P, o.aff_neg(P)], R - 5), ([P, o.aff_neg(P), Q, Q], rng.randrange(R))]
    at = 8
    for members, k in groups:
        for pt in members:
            pts[64 * at:64 * at + 64] = bytes(64) if pt is None else o.encode_affine_h2c(pt)
            sc[32 * at:32 * at + 32] = o.encode_scalar_h2c(k)
            at += 1
    return bytes(sc), bytes(pts)


def all_equal(n, seed):
    """every scalar the same: one bucket per window holds all n bases; a repeated base and an opposite pair among them"""
    pts = bytearray(co.gen_instance(o.SEED_BASE + 9200 + seed, n)[0])
    pts[64 * 3:64 * 4] = pts[64 * 2:64 * 3]                       # a base twice, next to itself
    y = int.from_bytes(pts[64 * 5 + 32:64 * 6], "little")
    pts[64 * 6:64 * 6 + 32] = pts[64 * 5:64 * 5 + 32]             # P and -P (Montgomery residues: -y = p - y)
    pts[64 * 6 + 32:64 * 7] = ((o.P - y) % o.P).to_bytes(32, "little")
    pts[64 * 9:64 * 10] = bytes(64)                               # an identity
    k = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCD % R
    return o.encode_scalar_h2c(k) * n, bytes(pts)


@pytest.fixture(scope="module")
def instances():
    """name, n -> (scalars, points, the oracle's affine result), computed once"""
    out = {}
    for n in SIZES:
        for name, make in (("planted", planted), ("all_equal", all_equal)):
            sc, pts = make(n, n)
            out[name, n] = (sc, pts, decode(co.msm_best(sc, pts, n, 2)))
    return out


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_msm_in_place_and_prepared(cfg, msm_pkg, instances, n, c):
    for name in ("planted", "all_equal"):
        sc, pts, want = instances[name, n]
        ds, dp = cfg.alloc(len(sc)), cfg.alloc(len(pts))
        prep = None
        try:
            cfg.to_device(ds, sc)
            cfg.to_device(dp, pts)
            cfg.set_window_size(c)
            in_place = cfg.msm_batch_device([ds], [dp], [n])[0]
            assert cfg.timings().window_size == c
            prep = cfg.bases_prepare_device(dp, n)
            packed = cfg.msm_batch_device([ds], [prep], [n], point_layout=msm_pkg.POINT_PREPARED)[0]
        finally:
            cfg.set_window_size(0)
            for d in (ds, dp, prep):
                if d is not None:
                    cfg.free(d)
        assert decode(in_place) == want, (name, "gathered in place")
        assert decode(packed) == want, (name, "prepared bases")
        assert in_place == packed, name


@pytest.mark.parametrize("square", [False, True], ids=["mul_sub", "sqr_sub"])
def test_folded_forms_device_equals_host(cfg, msm_pkg, square):
    op = host.FE_SQR_SUB if square else host.FE_MUL_SUB
    for sel in host.KSELS:
        recs = [host.fold_record(sel, a, b, x) for a, b, x in host.corpus(sel, square)]
        a = [w for r in recs for w in r[0]]
        b = [w for r in recs for w in r[1]]
        assert cfg.test_op_raw(op, a, b, len(recs)) == msm_pkg.test_op_raw_host(op, a, b, len(recs)), sel
