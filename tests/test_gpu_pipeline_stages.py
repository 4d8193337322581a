"""Stage tests of the shipped pipeline: digits, sort, work-item plan, accumulate, combine and window reduction, each
read through the stage tap (msm_amd_test_last_plan / msm_amd_test_stage_copy / msm_amd_test_fill_workspaces) after an
ordinary call, and each compared with a plain reference of that stage alone:

  digits        oracle.bn254_ref.signed_digits (vectorised here, checked against it)
  sort / plan   numpy restatements of the invariants (bucket sizes, scans, slot contents as sets, item order)
  buckets       oracle/msm_oracle.c: bucket sums of the oracle's digits, and a replay of the accumulate kernel's
                state machine that counts which branch every step takes
  partials      oracle/msm_oracle.c: bit-k subset sums over the slot index, the window total, sum (s + 1) B_s

Environment switches of the plan (MSM_AMD_HB, _MB, _TILED, _BALLOT, _LOW_OCC) appear in the test ids."""
import json
import os
import random

import numpy as np
import pytest

from oracle import bn254_ref as o
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


# ---- instances and the tap ----------------------------------------------------------------------------------------
def _mont_bytes(ks):
    return b"".join(o.encode_scalar_h2c(k) for k in ks)


def _canon_bytes(ks):
    return b"".join(int(k).to_bytes(32, "little") for k in ks)


def _run(cfg, msm_pkg, insts, c=0, canonical=False):
    """One call over device-resident buffers: insts = [(scalars (ints), points64 bytes)], a batch when more than one.
    Scalars go in Montgomery form, or canonical as given (values >= r included).  Returns the 96-byte results."""
    ptrs = []
    try:
        ds, dp, ns = [], [], []
        for ks, pts in insts:
            sb = _canon_bytes(ks) if canonical else _mont_bytes(ks)
            d_s, d_p = cfg.alloc(len(sb)), cfg.alloc(len(pts))
            ptrs += [d_s, d_p]
            cfg.to_device(d_s, sb)
            cfg.to_device(d_p, pts)
            ds.append(d_s)
            dp.append(d_p)
            ns.append(len(ks))
        cfg.set_window_size(c)
        return cfg.msm_batch_device(ds, dp, ns, msm_pkg.SCALAR_CANON_LE if canonical else msm_pkg.SCALAR_MONT_LE)
    finally:
        cfg.set_window_size(0)
        for p in ptrs:
            cfg.free(p)


def _expected(ks, pts):
    return co.msm_best(_mont_bytes(ks), pts, len(ks), 2)


def _same_point(a96, b96):
    return o.decode_jacobian_mont_le(a96) == o.decode_jacobian_mont_le(b96)


def _u32(cfg, msm_pkg, which, j=0):
    return np.frombuffer(cfg.test_stage_copy(which, j), dtype=np.uint32)


def _tap_digits(cfg, msm_pkg, plan, j=0):
    raw = cfg.test_stage_copy(msm_pkg.STAGE_DIGITS, j)
    dt, bits = (np.uint32, 32) if plan["wide_digits"] else (np.uint16, 16)
    v = np.frombuffer(raw, dtype=dt)
    d = (v & dt((1 << (bits - 1)) - 1)).astype(np.int32)
    np.negative(d, out=d, where=(v >> dt(bits - 1)) != 0)
    return d.reshape(plan["W_digits"], plan["n_scalars"])


def _be32_to_jac(raw):
    """Wire layout (3 x 8 u32, most significant first) -> the oracle's 96-byte Jacobian records."""
    a = np.frombuffer(raw, dtype=np.uint32).reshape(-1, 3, 8)[:, :, ::-1]
    return np.ascontiguousarray(a).tobytes()


def np_signed_digits(ks, c, W):
    """signed_digits for many scalars at once (numpy over 4 x u64 limbs of k mod r)."""
    n = len(ks)
    limbs = np.frombuffer(b"".join((k % o.R_ORDER).to_bytes(32, "little") for k in ks), dtype="<u8").reshape(n, 4)
    limbs = np.concatenate([limbs, np.zeros((n, 1), dtype=np.uint64)], axis=1)
    mask, half = np.uint64((1 << c) - 1), (1 << (c - 1))
    out = np.zeros((W, n), dtype=np.int64)
    carry = np.zeros(n, dtype=np.int64)
    for w in range(W):
        s = c * w
        li, off = s // 64, s % 64
        if li >= 4:
            v = np.zeros(n, dtype=np.uint64)
        else:
            v = limbs[:, li] >> np.uint64(off)
            if off + c > 64:
                v = v | (limbs[:, li + 1] << np.uint64(64 - off))
        v = (v & mask).astype(np.int64) + carry
        neg = v > half
        out[w] = np.where(neg, v - (1 << c), v)
        carry = neg.astype(np.int64)
    return out.astype(np.int32)


def _points(seed, m):
    return co.gen_instance(seed, m)[0]


def _rec_to_aff(rec):
    x, y = int.from_bytes(rec[:32], "little"), int.from_bytes(rec[32:64], "little")
    if x == 0 and y == 0:
        return None
    return (o.fq_from_mont(x), o.fq_from_mont(y))


def _edge_scalars(c, rng):
    W = o.MODULUS_BIT_SIZE // c + 1
    half = 1 << (c - 1)
    ks = [0, 1, 2, o.R_ORDER - 1, o.R_ORDER - 2, (1 << 14) + 1, (1 << 14) - 1]
    for w in range(1, W):
        if c * w < 254:
            ks += [(1 << (c * w)) - 1, (1 << (c * w)) + 1, 1 << (c * w), (half + 1) << (c * (w - 1))]
        if c * w + c <= 250:   # a raw window value of exactly 2^(c-1) stays positive: alone, and as a chain below 2^250
            ks += [half << (c * w), sum(half << (c * v) for v in range(w + 1))]
    ks.append(sum(half << (c * w) for w in range(W)) % o.R_ORDER)
    ks.append(sum((half + 1) << (c * w) for w in range(W)) % o.R_ORDER)
    ks.append(sum((half + (w & 1)) << (c * w) for w in range(W)) % o.R_ORDER)
    ks.append(sum((half - 1 + 2 * (w & 1)) << (c * w) for w in range(W)) % o.R_ORDER)
    return ks


# ---- digits ---------------------------------------------------------------------------------------------------------
def test_np_signed_digits_matches_oracle():
    rng = random.Random(3)
    for c in (3, 8, 13, 17, 24):
        ks = _edge_scalars(c, rng) + [rng.randrange(o.R_ORDER) for _ in range(50)]
        W = o.MODULUS_BIT_SIZE // c + 1
        got = np_signed_digits(ks, c, W)
        for t, k in enumerate(ks):
            assert list(got[:, t]) == o.signed_digits(k % o.R_ORDER, c, W)


@pytest.mark.parametrize("layout", ["mont", "canonical"])
@pytest.mark.parametrize("c", [3, 4, 5, 8, 13, 15, 16, 17])
def test_digits_exact(cfg, msm_pkg, c, layout):
    """digits_kernel<D, C>: the four specialisations (13, 15, 16, 17), the generic u16 / u32 forms and the padded c = 3,
    digit for digit against the oracle, edge scalars and carry chains included; canonical inputs also in [r, 2^256)."""
    rng = random.Random(c * 7 + (layout == "canonical"))
    ks = _edge_scalars(c, rng) + [rng.randrange(o.R_ORDER) for _ in range(1500)]
    if layout == "canonical":
        ks += [o.R_ORDER, o.R_ORDER + 1, (1 << 256) - 1, 5 * o.R_ORDER + 3, (1 << 255) + 12345]
        ks += [rng.randrange(o.R_ORDER, 1 << 256) for _ in range(200)]
    n = len(ks)
    pts = _points(o.SEED_BASE + c, n)
    out = _run(cfg, msm_pkg, [(ks, pts)], c=c, canonical=layout == "canonical")[0]
    plan = cfg.test_last_plan()
    W = o.MODULUS_BIT_SIZE // c + 1
    assert (plan["c"], plan["W_digits"], plan["n_scalars"], plan["wide_digits"]) == (c, W, n, int(c > 15))
    got = _tap_digits(cfg, msm_pkg, plan)
    exp = np_signed_digits(ks, c, W)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"first wrong digit (window, scalar) {tuple(bad[0])}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"
    assert _same_point(out, _expected([k % o.R_ORDER for k in ks], pts))


# ---- sort and plan invariants ---------------------------------------------------------------------------------------
def check_sort_plan(cfg, msm_pkg, digits, j=0, windows=None):
    """Every invariant of the sort / planning stage for instance j against a digit matrix [W][n], in numpy."""
    p = cfg.test_last_plan(j)
    W, n, nb, lb, CH = p["W"], p["n"], p["nb"], p["lb"], p["CH"]
    d = digits.reshape(W, n)
    mag = np.abs(d)
    size = _u32(cfg, msm_pkg, msm_pkg.STAGE_BUCKET_SIZE, j).reshape(W, nb).astype(np.int64)
    start = _u32(cfg, msm_pkg, msm_pkg.STAGE_BUCKET_START, j).reshape(W, nb).astype(np.int64)
    istart = _u32(cfg, msm_pkg, msm_pkg.STAGE_ITEM_START, j).reshape(W, nb).astype(np.int64)
    wbase = _u32(cfg, msm_pkg, msm_pkg.STAGE_WIN_ITEMS, j).astype(np.int64)
    srt = _u32(cfg, msm_pkg, msm_pkg.STAGE_SORTED, j).reshape(W, n)
    order = _u32(cfg, msm_pkg, msm_pkg.STAGE_ORDER, j).reshape(-1, 2).astype(np.int64)
    multi = _u32(cfg, msm_pkg, msm_pkg.STAGE_MULTI_LIST, j).astype(np.int64)
    items = (size + CH - 1) // CH
    for w in range(W):
        exp_size = np.bincount(mag[w], minlength=nb + 1)[1:]
        assert len(exp_size) == nb, f"window {w}: a digit magnitude above 2^lb"
        assert np.array_equal(size[w], exp_size), f"window {w}: bucket sizes"
        assert np.array_equal(start[w], np.cumsum(size[w]) - size[w]), f"window {w}: bucket_start"
        assert np.array_equal(istart[w], np.cumsum(items[w]) - items[w]), f"window {w}: item_start"
    assert np.array_equal(wbase, np.cumsum(items.sum(axis=1)) - items.sum(axis=1)), "window bases of the items"
    for w in (range(W) if windows is None else windows):
        nz = np.nonzero(mag[w])[0]
        cnt = len(nz)
        assert cnt == size[w].sum()
        exp_entries = nz.astype(np.uint64) | ((d[w, nz] < 0).astype(np.uint64) << np.uint64(31))
        exp_keys = np.sort((mag[w, nz].astype(np.uint64) - np.uint64(1)) << np.uint64(32) | exp_entries)
        slot_of = np.repeat(np.arange(nb, dtype=np.uint64), size[w])
        got_keys = np.sort(slot_of << np.uint64(32) | srt[w, :cnt].astype(np.uint64))
        assert np.array_equal(got_keys, exp_keys), f"window {w}: slot contents of `sorted`"
    total_items = int(items.sum())
    assert p["total_items"] == total_items and len(order) == total_items
    flat = size.reshape(-1)
    b, jj = order[:, 0], order[:, 1]
    assert np.all(b < W * nb) and np.all(jj < (flat[b] + CH - 1) // CH)
    keys = np.sort(b * 65536 * 64 + jj)
    assert len(np.unique(keys)) == total_items, "order: an item twice"
    length = np.minimum(flat[b] - jj * CH, CH)
    assert np.all(length[1:] <= length[:-1]), "order: item length increases"
    exp_multi = np.nonzero(items.reshape(-1) > 1)[0]
    assert p["multi_count"] == len(exp_multi)
    assert np.array_equal(np.sort(multi), exp_multi), "multi_list"
    return p


SORT_CASES = [
    # (id, log_n, c, env, expect)   expect: plan fields the case is meant to reach
    ("two_level_2p12_c8", 12, 8, {}, {"mb": 0}),
    ("two_level_2p15_c15", 15, 15, {}, {"mb": 0}),
    ("three_level_2p16_c15-HB2-MB2", 16, 15, {"MSM_AMD_HB": "2", "MSM_AMD_MB": "2"}, {"mb": 2, "hb": 2}),
    ("three_level_2p14_c13-HB1-MB2-TILED1", 14, 13, {"MSM_AMD_HB": "1", "MSM_AMD_MB": "2", "MSM_AMD_TILED": "1"},
     {"mb": 2, "tiled": 1}),
    ("three_level_2p16_c17-HB3-MB3-TILED0", 16, 17, {"MSM_AMD_HB": "3", "MSM_AMD_MB": "3", "MSM_AMD_TILED": "0"},
     {"mb": 3, "tiled": 0}),
    ("two_level_2p15_c16-TILED1", 15, 16, {"MSM_AMD_TILED": "1"}, {"mb": 0, "tiled": 1}),
] + [(f"two_level_2p14_c15-BALLOT{b}", 14, 15, {"MSM_AMD_BALLOT": str(b)}, {"ballot": b}) for b in range(4)] + [
    (f"three_level_2p15_c15-HB2-MB2-BALLOT{b}", 15, 15, {"MSM_AMD_HB": "2", "MSM_AMD_MB": "2", "MSM_AMD_BALLOT": str(b)},
     {"ballot": b, "mb": 2}) for b in (0, 3)]


@pytest.mark.parametrize("case", SORT_CASES, ids=[c[0] for c in SORT_CASES])
def test_sort_and_plan(cfg, msm_pkg, monkeypatch, case):
    _id, log_n, c, env, expect = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 1 << log_n
    rng = random.Random(log_n * 31 + c)
    ks = [rng.randrange(o.R_ORDER) for _ in range(n - 64)] + _edge_scalars(c, rng)[:64]
    pts = _points(o.SEED_BASE + log_n, len(ks))
    _run(cfg, msm_pkg, [(ks, pts)], c=c)
    plan = cfg.test_last_plan()
    for k, v in expect.items():
        assert plan[k] == v, f"plan does not take the intended path: {k} = {plan[k]} ({plan})"
    digits = _tap_digits(cfg, msm_pkg, plan)
    assert np.array_equal(digits, np_signed_digits(ks, c, plan["W_digits"]))
    check_sort_plan(cfg, msm_pkg, digits)


def test_sort_fine_fallback_and_big_split(cfg, msm_pkg):
    """40 000 equal scalars: every window's points share one slot, so the fine-sort region exceeds kFineCap (28 672)
    and the pass-2 fallback scatters in global memory; the bucket is cut into > 8 items (combine_big_kernel)."""
    n = 40000
    k = 0x1234_5678_9ABC_DEF0_1357_9BDF_0246_8ACE
    ks = [k] * n
    pts = _points(o.SEED_BASE + 40000, n)
    out = _run(cfg, msm_pkg, [(ks, pts)], c=15)[0]
    plan = cfg.test_last_plan()
    digits = _tap_digits(cfg, msm_pkg, plan)
    check_sort_plan(cfg, msm_pkg, digits)
    assert plan["deferred"] > 0
    assert _same_point(out, _expected(ks, pts))


def test_sort_default_plan_2p22(cfg, msm_pkg):
    """The default plan of a lone 2^22-point call picks the three-level, tiled sort on its own."""
    n = 1 << 22
    dp, ds = cfg.generate_instance(o.SEED_BASE + 22, n, True)
    try:
        cfg.msm_batch_device([ds], [dp], [n])
    finally:
        cfg.free(dp)
        cfg.free(ds)
    plan = cfg.test_last_plan()
    assert plan["lone"] == 1 and plan["mb"] > 0 and plan["tiled"] == 1, plan
    digits = _tap_digits(cfg, msm_pkg, plan)
    check_sort_plan(cfg, msm_pkg, digits, windows=[0, plan["W"] // 2, plan["W"] - 1])


# ---- accumulate and combine -----------------------------------------------------------------------------------------
CLASS_COUNTS = {"ship": {}, "low_occ0": {}}


def check_buckets(cfg, msm_pkg, ks, pts, out, c, j=0, counts=None):
    """Every non-empty bucket of instance j against the oracle's bucket sums; the window partials; the result.
    counts: a dict that receives the replayed branch classes of the accumulate kernel."""
    p = cfg.test_last_plan(j)
    assert p["c"] == c
    W, nb, lb, n = p["W"], p["nb"], p["lb"], p["n"]
    digits = np_signed_digits(ks, c, p["W_digits"])
    tap = _tap_digits(cfg, msm_pkg, p, j)
    assert np.array_equal(tap, digits)
    size = _u32(cfg, msm_pkg, msm_pkg.STAGE_BUCKET_SIZE, j)
    exp_size = np.stack([np.bincount(np.abs(digits[w]), minlength=nb + 1)[1:] for w in range(W)])
    assert np.array_equal(size, exp_size.reshape(-1)), "bucket sizes"
    exp_b = co.stage_buckets(digits, pts, lb)
    got_b = _be32_to_jac(cfg.test_stage_copy(msm_pkg.STAGE_BUCKETS, j))
    bad, first = co.jac_mismatches(got_b, exp_b, size != 0)
    assert bad == 0, f"{bad} buckets differ; first: window {first >> lb} slot {first & (nb - 1)} size {size[first]}"
    exp_part, _ = co.stage_partials(exp_b, W, lb)
    got_part = _be32_to_jac(cfg.test_stage_copy(msm_pkg.STAGE_PARTIAL, j))
    bad, first = co.jac_mismatches(got_part, exp_part)
    assert bad == 0, f"{bad} window partials differ; first: window {first // (lb + 1)} term {first % (lb + 1)}"
    assert _same_point(out, _expected(ks, pts))
    if counts is not None:
        srt = _u32(cfg, msm_pkg, msm_pkg.STAGE_SORTED, j)
        start = _u32(cfg, msm_pkg, msm_pkg.STAGE_BUCKET_START, j)
        got = co.replay_items(srt, start, size, n, W, lb, p["CH"], pts)
        for k, v in got.items():
            counts[k] = counts.get(k, 0) + v
        counts["multi_count"] = counts.get("multi_count", 0) + p["multi_count"]
        counts["deferred"] = counts.get("deferred", 0) + p["deferred"]
    return p


def _reference_lists():
    with open(os.path.join(GOLDEN, "reference_index_lists.json")) as f:
        cases = json.load(f)["bucket_wise_accumulation"]
    assert len(cases) == 16
    return [[tuple(pr) for pr in case["buckets_indices"]] for case in cases]


@pytest.fixture(scope="module")
def ctx_low_occ0(msm_pkg):
    """A ctx whose accumulate launches run accumulate_kernel<false> (MSM_AMD_LOW_OCC=0 is read at init)."""
    old = os.environ.get("MSM_AMD_LOW_OCC")
    os.environ["MSM_AMD_LOW_OCC"] = "0"
    try:
        c = msm_pkg.MsmConfig(0)
    finally:
        if old is None:
            del os.environ["MSM_AMD_LOW_OCC"]
        else:
            os.environ["MSM_AMD_LOW_OCC"] = old
    yield c
    c.close()


def _ctx(kernel, cfg, ctx_low_occ0):
    return cfg if kernel == "ship" else ctx_low_occ0


@pytest.mark.parametrize("kernel", ["ship", "low_occ0"], ids=["ship", "MSM_AMD_LOW_OCC0"])
@pytest.mark.parametrize("c,negative", [(9, False), (10, True)])
def test_accumulate_reference_lists(cfg, ctx_low_occ0, msm_pkg, kernel, c, negative):
    """The reference's 16 index lists as one-window inputs: pair (beta, i) is its own point slot with base P_i and
    scalar beta + 1 (a duplicate pair puts one base twice into a bucket); the negative twin uses 2^c - (beta + 1),
    digit -(beta + 1) with a carry that puts every point into slot 0 of window 1 (one large split bucket)."""
    ctx = _ctx(kernel, cfg, ctx_low_occ0)
    for li, pairs in enumerate(_reference_lists()):
        npts = max(i for _, i in pairs) + 1
        base = _points(o.SEED_BASE + 1000 + li, npts)
        pts = b"".join(base[64 * i:64 * i + 64] for _, i in pairs)
        ks = [((1 << c) - (b + 1)) if negative else b + 1 for b, _ in pairs]
        assert max(b + 1 for b, _ in pairs) <= (1 << (c - 1)) - (1 if negative else 0)
        out = _run(ctx, msm_pkg, [(ks, pts)], c=c)[0]
        p = check_buckets(ctx, msm_pkg, ks, pts, out, c, counts=CLASS_COUNTS[kernel])
        if not negative:   # the stand-in test's oracle, bucket by bucket of window 0
            pj = [o.to_jac(_rec_to_aff(base[64 * i:64 * i + 64])) for i in range(npts)]
            exp = o.bucket_wise_accumulation(pairs, pj)
            got = ctx.test_stage_copy(msm_pkg.STAGE_BUCKETS)
            size = _u32(ctx, msm_pkg, msm_pkg.STAGE_BUCKET_SIZE)
            for b, e in enumerate(exp):
                if size[b]:
                    dec = o.decode_point_be32(np.frombuffer(got[96 * b:96 * b + 96], dtype=np.uint32).tolist())
                    assert (o.to_affine(dec) if dec else None) == o.to_affine(e), f"list {li} bucket {b}"
        assert p["W"] == o.MODULUS_BIT_SIZE // c + 1


@pytest.mark.parametrize("kernel", ["ship", "low_occ0"], ids=["ship", "MSM_AMD_LOW_OCC0"])
@pytest.mark.parametrize("negative", [False, True])
def test_accumulate_reference_lists_c17(cfg, ctx_low_occ0, msm_pkg, kernel, negative):
    """The 16 lists at c = 17 in one instance (list k owns slots 256 k .. 256 k + 255)."""
    ctx = _ctx(kernel, cfg, ctx_low_occ0)
    c = 17
    ks, recs = [], []
    for li, pairs in enumerate(_reference_lists()):
        npts = max(i for _, i in pairs) + 1
        base = _points(o.SEED_BASE + 1000 + li, npts)
        for b, i in pairs:
            v = 256 * li + b + 1
            ks.append((1 << c) - v if negative else v)
            recs.append(base[64 * i:64 * i + 64])
    pts = b"".join(recs)
    out = _run(ctx, msm_pkg, [(ks, pts)], c=c)[0]
    check_buckets(ctx, msm_pkg, ks, pts, out, c, counts=CLASS_COUNTS[kernel])


def constructed_instance(seed=7):
    """One-window (c = 9) input whose buckets reach every branch of accumulate_item and of the combine kernels in any
    order the sort leaves inside a bucket.  Returns (scalars, points64)."""
    rng = random.Random(seed)
    pool = _points(o.SEED_BASE + 5000 + seed, 200)
    aff = [_rec_to_aff(pool[64 * i:64 * i + 64]) for i in range(200)]
    enc = o.encode_affine_h2c
    ks, recs = [], []
    nxt = iter(range(200))

    def bucket(v, points, negative=False):
        assert 1 <= v <= 255
        for pt in points:
            ks.append(512 - v if negative else v)   # negative: digit -v, carry into window 1
            recs.append(enc(pt))

    P = lambda: aff[next(nxt)]
    v = iter(range(1, 256))
    p = P()
    bucket(next(v), [p, p])                                   # phase A doubling
    p = P()
    bucket(next(v), [p, p], negative=True)                    # ... of a negated base (regather keeps the sign)
    p = P()
    bucket(next(v), [p, p, p, p])                             # a multiset of one base
    p = P()
    bucket(next(v), [p, o.aff_neg(p)])                        # cancellation from kOne
    p, q = P(), P()
    bucket(next(v), [p, o.aff_neg(p), q], negative=True)      # ... then a restart
    for _ in range(3):
        p, q, r = P(), P(), P()
        bucket(next(v), [p, q, o.aff_neg(o.aff_add(p, q))])    # cancellation in phase B
        p, q, r = P(), P(), P()
        bucket(next(v), [p, q, o.aff_neg(o.aff_add(p, q)), r], negative=True)   # ... then a restart
    for i in range(48):                                       # phase B doubling for the order (P, P, 2P)
        p = P() if i < 40 else aff[i]
        bucket(next(v), [p, p, o.aff_add(p, p)], negative=bool(i & 1))
    bucket(next(v), [None, None, P()])                        # identity bases
    bucket(next(v), [None])
    for size in (15, 16, 17):                                 # CH - 1, CH, CH + 1 (CH = 16, asserted)
        bucket(next(v), [aff[rng.randrange(200)] for _ in range(size)], negative=size == 17)
    bucket(next(v), [None] * 32)                              # split bucket whose items sum to the identity
    p, q = P(), P()
    bucket(next(v), [p] * 16 + [q, o.aff_neg(q)] * 8)         # split bucket: items 16 P / identity in some order
    p = P()
    bucket(next(v), [p] * 32, negative=True)                  # split bucket, all partials equal: doubling in pti_add
    p = P()
    bucket(next(v), [p] * 128)                                # 8 CH: combine_small, kSerialItems items
    bucket(next(v), [aff[rng.randrange(200)] for _ in range(129)])   # 8 CH + 1: combine_big
    bucket(next(v), [aff[rng.randrange(200)] for _ in range(1100)], negative=True)   # > 64 CH: strided loop + tree
    p = P()
    bucket(next(v), [p] * 1040)                               # 65 equal items: doubling inside the LDS tree
    return ks, b"".join(recs)


@pytest.fixture(scope="module")
def constructed():
    return constructed_instance()


@pytest.mark.parametrize("kernel", ["ship", "low_occ0"], ids=["ship", "MSM_AMD_LOW_OCC0"])
def test_accumulate_constructed_buckets(cfg, ctx_low_occ0, msm_pkg, constructed, kernel):
    ctx = _ctx(kernel, cfg, ctx_low_occ0)
    ks, pts = constructed
    out = _run(ctx, msm_pkg, [(ks, pts)], c=9)[0]
    p = ctx.test_last_plan()
    assert p["CH"] == 16, "the constructed bucket sizes assume CH = 16"
    assert p["multi_count"] > 0 and p["deferred"] > 0
    check_buckets(ctx, msm_pkg, ks, pts, out, 9, counts=CLASS_COUNTS[kernel])


@pytest.mark.parametrize("kernel", ["ship", "low_occ0"], ids=["ship", "MSM_AMD_LOW_OCC0"])
def test_branch_classes_all_reached(cfg, ctx_low_occ0, msm_pkg, constructed, kernel):
    """The coverage claim as a test: over this file's accumulate inputs every branch class of accumulate_item occurred,
    and both combine kernels ran.  (Runs the constructed input itself when the tests above were deselected.)"""
    counts = CLASS_COUNTS[kernel]
    if not counts:
        ctx = _ctx(kernel, cfg, ctx_low_occ0)
        ks, pts = constructed
        out = _run(ctx, msm_pkg, [(ks, pts)], c=9)[0]
        check_buckets(ctx, msm_pkg, ks, pts, out, 9, counts=counts)
    print(f"\nbranch classes ({kernel}): " + ", ".join(f"{k}={v}" for k, v in counts.items()))
    missing = [k for k in co.STEP_CLASSES + ("multi_count", "deferred") if counts.get(k, 0) == 0]
    assert not missing, f"branch classes never reached: {missing} ({counts})"


# ---- window partials: lone and pipelined reduce geometry ------------------------------------------------------------
def _window_identity(part_be32, W, lb, window96):
    """partial[w][lb] + sum_k 2^k partial[w][k] == sum_s (s + 1) B[w][s] (host big-integer arithmetic)."""
    parts = np.frombuffer(part_be32, dtype=np.uint32).reshape(W, lb + 1, 24)
    for w in range(W):
        acc = o.decode_point_be32(parts[w, lb].tolist())
        for k in range(lb):
            t = o.decode_point_be32(parts[w, k].tolist())
            if t is not None:
                acc = o.jac_add(acc, o.scalar_mul_jac(1 << k, t))
        exp = o.decode_jacobian_mont_le(window96[96 * w:96 * w + 96])
        assert (o.to_affine(acc) if acc else None) == exp, f"window {w}: weighted partials"


@pytest.mark.parametrize("n_inst", [1, 3], ids=["lone", "pipelined3"])
def test_window_partials(cfg, msm_pkg, n_inst):
    c = 8
    insts = []
    for i in range(n_inst):
        rng = random.Random(100 + i)
        n = 3000 + 500 * i
        ks = [rng.randrange(o.R_ORDER) for _ in range(n - 40)] + _edge_scalars(c, rng)[:40]
        insts.append((ks, _points(o.SEED_BASE + 200 + i, n)))
    outs = _run(cfg, msm_pkg, insts, c=c)
    for j, (ks, pts) in enumerate(insts):
        p = check_buckets(cfg, msm_pkg, ks, pts, outs[j], c, j=j)
        if n_inst == 1:
            assert p["lone"] == 1 and p["rb_threads"] == 0 and p["red_group"] < 16
        else:
            assert p["lone"] == 0 and p["rb_threads"] == 64 and p["red_group"] == 16
        if j == 0:
            digits = np_signed_digits(ks, c, p["W_digits"])
            _, win = co.stage_partials(co.stage_buckets(digits, pts, p["lb"]), p["W"], p["lb"])
            _window_identity(cfg.test_stage_copy(msm_pkg.STAGE_PARTIAL, j), p["W"], p["lb"], win)
    assert len({cfg.test_last_plan(j)["workspace"] for j in range(n_inst)}) == n_inst


def test_tap_refuses_large_batch(cfg, msm_pkg):
    rng = random.Random(9)
    insts = [([rng.randrange(o.R_ORDER) for _ in range(64)], _points(o.SEED_BASE + 300 + i, 64)) for i in range(5)]
    _run(cfg, msm_pkg, insts, c=5)
    with pytest.raises(msm_pkg.MsmError) as e:
        cfg.test_last_plan(0)
    assert e.value.status == msm_pkg.INPUT_ERROR


# ---- stale workspaces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_poisoned_workspaces(cfg, msm_pkg, byte):
    """The bucket matrix is not cleared between calls: the window reduction must take every empty slot as the identity
    from bucket_size alone.  Point-valued workspace buffers are filled with a non-zero byte before every call of a
    sequence whose plans grow and shrink; every result must still equal the oracle."""
    rng = random.Random(byte)
    seq = []
    n = 4096
    seq.append(("c17", 17, [rng.randrange(o.R_ORDER) for _ in range(n)]))
    seq.append(("c3", 3, [rng.randrange(o.R_ORDER) for _ in range(40)]))
    seq.append(("c5_skewed", 5, [rng.choice([1, 2, 33, 1 << 200]) for _ in range(600)]))
    seq.append(("c15", 15, [rng.randrange(o.R_ORDER) for _ in range(2048)]))
    seq.append(("c16_skewed", 16, [rng.randrange(1 << 20) for _ in range(3000)]))
    seq.append(("zeros", 15, [0] * 512))
    seq.append(("c5", 5, [rng.randrange(o.R_ORDER) for _ in range(1000)]))
    seq.append(("c17_small", 17, [rng.randrange(o.R_ORDER) for _ in range(100)]))
    pts = _points(o.SEED_BASE + 400, n)
    for name, c, ks in seq:
        cfg.test_fill_workspaces(byte)
        out = _run(cfg, msm_pkg, [(ks, pts[:64 * len(ks)])], c=c)[0]
        assert cfg.test_last_plan()["c"] == c
        assert _same_point(out, _expected(ks, pts[:64 * len(ks)])), f"{name}: result differs after poisoning"
    # the precomputed-table pipeline (one window of W_digits * n entries, plan_tile_sums_kernel)
    tables = cfg.tables_build(pts[:64 * 2048], 2048, window_size=16)
    try:
        ks = [rng.randrange(o.R_ORDER) for _ in range(2048)]
        cfg.test_fill_workspaces(byte)
        out = cfg.msm_tables(_mont_bytes(ks), tables)
        p = cfg.test_last_plan()
        assert p["c"] == 16 and p["W"] == 1 and p["nb"] > 16384
        assert _same_point(out, _expected(ks, pts[:64 * 2048])), "tables: result differs after poisoning"
    finally:
        cfg.tables_free(tables)
