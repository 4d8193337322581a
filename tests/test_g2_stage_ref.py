"""CPU-only tests of the G2 stage reference (tests/g2_stage_ref.py): the discrete-log shortcuts against the big-integer
point model of tests/g2_ref.py, and the coverage claim of the constructed instance under any order inside a bucket."""
import random

import numpy as np
import pytest

import g2_ref as g
import g2_stage_ref as sr
import test_g2_host as th
from oracle import bn254_ref as o

CH = 16   # the chunk length the constructed bucket sizes assume (the GPU test asserts it from the plan)


def digit_matrix(ks, c):
    W = o.MODULUS_BIT_SIZE // c + 1
    return np.array([o.signed_digits(k % g.R_ORDER, c, W) for k in ks], dtype=np.int64).T.copy()


@pytest.fixture(scope="module")
def constructed():
    ks, dl = sr.constructed_instance()
    c = sr.CONSTRUCTED_C
    return ks, dl, digit_matrix(ks, c), c, c - 1


def replay_item_points(entries, points):
    """accumulate_g2_kernel's loop over one item on points of the model: the classes come from point comparisons"""
    EMPTY, ONE, MANY = 0, 1, 2
    state, acc, cancelled, classes = EMPTY, None, False, []
    for e in entries:
        base = points[e & 0x7FFFFFFF]
        if base is None:
            classes.append("identity_skip")
            continue
        q = g.neg(base) if e >> 31 else base
        if state == EMPTY:
            classes.append("restart_after_cancel" if cancelled else "first_point")
            state, acc = ONE, q
            continue
        where = "one" if state == ONE else "many"
        if q == acc:
            classes.append(where + "_double")
            state = MANY
        elif q == g.neg(acc):
            classes.append(where + "_cancel")
            state, cancelled = EMPTY, True
        else:
            classes.append(where + "_generic")
            state = MANY
        acc = g.add(acc, q)
    return classes, (None if state == EMPTY else acc)


def test_point_of_matches_scalar_mul():
    rng = random.Random(1)
    for s in [0, 1, 255, 256, 257, (1 << 40) - 1, g.R_ORDER - 1, g.R_ORDER, g.R_ORDER + 5, 3 * g.R_ORDER + 77,
              rng.randrange(1 << 50), rng.randrange(g.R_ORDER), rng.randrange(1 << 300)]:
        assert sr.point_of(s) == g.scalar_mul(s % g.R_ORDER, g.GEN2), s
        assert sr.point_of(-s) == g.neg(sr.point_of(s))
    assert g.on_curve(sr.point_of(123456789))


@pytest.mark.parametrize("perm_seed", [11, 12, 13])
def test_constructed_replay_dlogs_equal_points_and_reach_every_class(constructed, perm_seed):
    """Under a random order inside every bucket: the dlog replay and the point replay take the same class at every
    step and end every item at the same point, and every class of STEP_CLASSES occurs."""
    ks, dl, digits, c, lb = constructed
    W, n = digits.shape
    srt, start, size = sr.sort_reference(digits, lb, random.Random(perm_seed))
    points = [sr.point_of(a) if a else None for a in dl]
    counts = dict.fromkeys(sr.STEP_CLASSES, 0)
    items = 0
    for b, j, entries in sr.work_items(srt, start, size, n, W, lb, CH):
        cd, fd = sr.replay_item_dlog(entries, dl)
        cp, fp = replay_item_points(entries, points)
        assert cd == cp, f"bucket {b} item {j}: classes differ"
        assert (None if fd is None else sr.point_of(fd)) == fp, f"bucket {b} item {j}: final point"
        for k in cd:
            counts[k] += 1
        counts["item_identity"] += fd is None
        items += 1
    assert counts == sr.replay_items(srt, start, size, n, W, lb, CH, dl)
    missing = [k for k in sr.STEP_CLASSES if counts[k] == 0]
    assert not missing, f"classes never reached: {missing} ({counts})"
    per_bucket = (size.astype(np.int64) + CH - 1) // CH
    assert items == per_bucket.sum()
    assert (per_bucket > 1).any() and (per_bucket > 8).any(), "no split bucket / no bucket for combine_big"


def random_instance(seed, n, c):
    rng = random.Random(seed)
    dl = sr.distinct_dlogs(rng, n)
    dl[1] = 0                                     # an identity base
    ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
    ks[0], ks[2] = g.R_ORDER - 1, 0
    return ks, dl, digit_matrix(ks, c)


def test_partials_horner_is_the_msm(constructed):
    ks, dl, digits, c, lb = constructed
    cases = [(ks, dl, digits, c, lb)]
    rk, rd, rdig = random_instance(5, 24, 6)
    cases.append((rk, rd, rdig, 6, 5))
    for ks, dl, digits, c, lb in cases:
        sums, _ = sr.expected_buckets(digits, dl, lb)
        pd, pp = sr.expected_partials(sums, digits.shape[0], lb)
        total = sr.horner(pd, c, lb)
        assert total % g.R_ORDER == sum(k * a for k, a in zip(ks, dl)) % g.R_ORDER
        assert sr.point_of(total) == th.expected(ks, dl)
        # the weighted identity of one window: partial[w][lb] + sum 2^k partial[w][k] = sum (s + 1) B[w][s]
        for w, wv in enumerate(sr.window_values(sums)):
            assert pd[w][lb] + sum(pd[w][k] << k for k in range(lb)) == wv
        assert pp[0][lb] == sr.point_of(pd[0][lb])


def test_expected_buckets_against_point_sums():
    c, lb = 5, 4
    ks, dl, digits = random_instance(9, 40, c)
    dl[7] = dl[6]                                   # equal and opposite bases in the mix
    dl[9] = g.R_ORDER - dl[8]
    sums, pts = sr.expected_buckets(digits, dl, lb)
    base = [sr.point_of(a) if a else None for a in dl]
    W, n = digits.shape
    seen = 0
    for w in range(W):
        direct = {}
        for i in range(n):
            v = int(digits[w, i])
            if v:
                direct[abs(v) - 1] = g.add(direct.get(abs(v) - 1), base[i] if v > 0 else g.neg(base[i]))
        assert direct == pts[w], f"window {w}"
        seen += len(direct)
    assert seen > 200
    # and the partials of those buckets, as points, against subset sums of the direct buckets of one window
    _, pp = sr.expected_partials(sums, W, lb)
    for k in range(lb + 1):
        acc = None
        for s, pt in pts[3].items():
            if k == lb or (s >> k) & 1:
                acc = g.add(acc, pt)
        assert acc == pp[3][k]


def test_decode_records_identity_and_subset():
    pt = sr.point_of(99)
    one = o.fq_to_mont(1).to_bytes(32, "little")
    stale = b"\xa5" * 128 + bytes(64)                      # any x, y with z all zero is the identity
    rec = g.identity_bytes() + stale + g.encode_h2c(pt) + one + bytes(32)
    assert sr.decode_records(rec) == [None, None, pt]
    assert sr.decode_records(rec, which=[2]) == [..., ..., pt]
