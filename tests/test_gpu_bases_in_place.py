"""G1 MSMs whose bases are gathered in place from the caller's external records (no conversion pass): the instance runs
on the isomorphic curve E' and is mapped back on the host (csrc/bn254_ec29.hip.h, msm_host.hip).  Every comparison is
equality of the canonical affine point or of the 96 result bytes against oracle.c_oracle.msm_best / oracle.bn254_ref."""
import random

import numpy as np
import pytest

import test_bases_in_place_host as host
import test_gpu_pipeline_stages as ps
from oracle import bn254_ref as o
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
R = o.R_ORDER


def mont(ks):
    return b"".join(o.encode_scalar_h2c(k) for k in ks)


def all_negative(c):
    """every window's digit is negative: raw window value 2^(c-1) + 1 everywhere"""
    W = o.MODULUS_BIT_SIZE // c + 1
    return sum(((1 << (c - 1)) + 1) << (c * w) for w in range(W)) % R


def scalars_for(n, seed):
    rng = random.Random(seed)
    ks = [R - 1, 0, 1, all_negative(3), all_negative(8), all_negative(13), all_negative(17), 2, R - 2]
    return (ks + [rng.randrange(R) for _ in range(max(0, n - len(ks)))])[:n]


class Device:
    """buffers on the device for the length of one test"""

    def __init__(self, cfg):
        self.cfg, self.ptrs = cfg, []

    def put(self, data):
        d = self.cfg.alloc(len(data))
        self.ptrs.append(d)
        self.cfg.to_device(d, data)
        return d

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.cfg.set_window_size(0)
        for p in self.ptrs:
            self.cfg.free(p)


def decode(out96):
    return o.decode_jacobian_mont_le(out96)


@pytest.fixture(scope="module")
def pool():
    """1000 bases and the oracle's results for the prefixes the tests use, computed once"""
    pts = co.gen_instance(o.SEED_BASE + 7100, 1000)[0]
    want = {}
    for n in (1, 2, 3, 64, 65, 1000):
        ks = scalars_for(n, n)
        want[n] = (ks, decode(co.msm_best(mont(ks), pts[:64 * n], n, 2)))
    return pts, want


# ---- 1. small MSMs through the in-place path ------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 8, 13, 0], ids=["c3", "c8", "c13", "auto"])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_small_msm_device_resident_h2c(cfg, msm_pkg, pool, n, c):
    pts, want = pool
    ks, exp = want[n]
    with Device(cfg) as d:
        ds, dp = d.put(mont(ks)), d.put(pts[:64 * n])
        cfg.set_window_size(c)
        out = cfg.msm_batch_device([ds], [dp], [n])[0]
        assert decode(out) == exp
        # 5. the caller's array is read, never written
        assert cfg.to_host(dp, 64 * n) == pts[:64 * n]


# ---- 2. identities ---------------------------------------------------------------------------------------------------
def test_identity_bases_inside_one_bucket(cfg, msm_pkg, pool):
    pts, _ = pool
    A, B, Z = pts[0:64], pts[64:128], bytes(64)
    for recs in ([Z, A, B], [A, Z, B], [A, B, Z], [Z, Z, A], [A, Z, Z], [Z, A, Z], [Z] * 3 + [A, B] + [Z] * 2):
        for k in (5, R - 5):   # one bucket of window 0, positive and negative digit
            ks = [k] * len(recs)
            p = b"".join(recs)
            with Device(cfg) as d:
                cfg.set_window_size(8)
                out = cfg.msm_batch_device([d.put(mont(ks))], [d.put(p)], [len(ks)])[0]
            assert decode(out) == decode(co.msm_best(mont(ks), p, len(ks), 2))


@pytest.mark.parametrize("n", [1, 3, 100])
def test_all_identity_instance_returns_the_identity(cfg, msm_pkg, n):
    ks = scalars_for(n, 3)[::-1]
    with Device(cfg) as d:
        out = cfg.msm_batch_device([d.put(mont(ks))], [d.put(bytes(64 * n))], [n])[0]
    assert decode(out) is None


# ---- 3. exceptional branches on E' ----------------------------------------------------------------------------------
def branch_instance():
    """One window (c = 9): the stage file's constructed instance, and ahead of it the buckets named here: one base twice
    and three times (doubling through regather), P then -P (vanish, restart from empty), P, -P, P."""
    ks, pts = ps.constructed_instance(seed=11)
    pool = ps._points(o.SEED_BASE + 7200, 8)
    aff = [ps._rec_to_aff(pool[64 * i:64 * i + 64]) for i in range(8)]
    enc = o.encode_affine_h2c
    extra_k, extra_p = [], []

    def bucket(v, points, negative=False):
        for pt in points:
            extra_k.append(512 - v if negative else v)
            extra_p.append(enc(pt))

    P, Q = aff[0], aff[1]
    used = set(k if k < 256 else 512 - k for k in ks)
    free = iter(v for v in range(1, 256) if v not in used)
    bucket(next(free), [P, P])
    bucket(next(free), [P, P, P])
    bucket(next(free), [Q, Q, Q], negative=True)
    bucket(next(free), [P, o.aff_neg(P)])
    bucket(next(free), [P, o.aff_neg(P), P])
    bucket(next(free), [Q, o.aff_neg(Q), Q], negative=True)
    bucket(next(free), [P, o.aff_neg(P), Q, Q])
    return extra_k + ks, b"".join(extra_p) + pts


@pytest.fixture(scope="module")
def branches():
    ks, pts = branch_instance()
    return ks, pts, co.msm_best(mont(ks), pts, len(ks), 2)


def test_exceptional_branches_bucket_by_bucket(cfg, msm_pkg, branches):
    ks, pts, _ = branches
    out = ps._run(cfg, msm_pkg, [(ks, pts)], c=9)[0]
    counts = {}
    ps.check_buckets(cfg, msm_pkg, ks, pts, out, 9, counts=counts)   # buckets and window partials read on E
    missing = [k for k in co.STEP_CLASSES if counts.get(k, 0) == 0]
    assert not missing, f"branch classes never reached: {missing} ({counts})"


# ---- 4. both instantiations agree -----------------------------------------------------------------------------------
def ark_affine(pts64):
    n = len(pts64) // 64
    rec = np.zeros((n, 72), dtype=np.uint8)
    src = np.frombuffer(pts64, dtype=np.uint8).reshape(n, 64)
    rec[:, :64] = src
    rec[:, 64] = (~src.any(axis=1)).astype(np.uint8)   # infinity flag
    return rec.tobytes()


def ark_projective(pts64):
    out = []
    for i in range(len(pts64) // 64):
        a = ps._rec_to_aff(pts64[64 * i:64 * i + 64])
        out.append(o.encode_projective_ark(None if a is None else (a[0], a[1], 1)))
    return b"".join(out)


def every_path(cfg, msm_pkg, ks, pts, c):
    """name -> 96 result bytes, over every way the same instance can be handed in"""
    n, sc = len(ks), mont(ks)
    res = {}
    with Device(cfg) as d:
        cfg.set_window_size(c)
        ds, dp = d.put(sc), d.put(pts)
        res["h2c in place"] = cfg.msm_batch_device([ds], [dp], [n])[0]
        res["ark affine"] = cfg.msm_batch_device([ds], [d.put(ark_affine(pts))], [n], point_layout=msm_pkg.POINT_ARK_AFFINE)[0]
        res["ark projective"] = cfg.msm_batch_device([ds], [d.put(ark_projective(pts))], [n],
                                                     point_layout=msm_pkg.POINT_ARK_PROJECTIVE)[0]
        prep = cfg.bases_prepare_device(dp, n)
        d.ptrs.append(prep)
        res["prepared"] = cfg.msm_batch_device([ds], [prep], [n], point_layout=msm_pkg.POINT_PREPARED)[0]
        res["host slices"] = cfg.msm_batch([sc, sc], [pts, pts], [n, n])[1]
        cfg.set_bases_cache(1 << 24)
        try:
            res["cache miss"] = cfg.msm_batch([sc], [pts], [n])[0]
            res["cache hit"] = cfg.msm_batch([sc], [pts], [n])[0]
            assert cfg.bases_cache_stats()["hits"] >= 1
        finally:
            cfg.set_bases_cache(0)
        cfg.set_window_size(0)
        tb = cfg.tables_build_device(dp, n)
        try:
            res["tables"] = cfg.msm_tables(sc, tb)
        finally:
            cfg.tables_free(tb)
    return res


@pytest.mark.parametrize("which", ["branches", "random1000"])
def test_every_record_kind_gives_the_same_bytes(cfg, msm_pkg, pool, branches, which):
    if which == "branches":
        ks, pts, want = branches
        c = 9
    else:
        pts, w = pool
        ks = w[1000][0]
        want, c = co.msm_best(mont(ks), pts, 1000, 2), 0
    res = every_path(cfg, msm_pkg, ks, pts, c)
    for name, out in res.items():
        assert decode(out) == decode(want), name
        assert out == res["h2c in place"], name


# ---- 6. lifetime ----------------------------------------------------------------------------------------------------
def test_two_batches_in_flight_then_the_workspaces_again(cfg, msm_pkg):
    """submit, submit, wait, wait with different bases per instance; a third batch then re-uses the first one's
    workspaces with new bases.  The callers' arrays are gathered until the wait: they stay as uploaded."""
    n, per = 4096, 2
    insts = []
    for i in range(3 * per):
        pts, sc = co.gen_instance(o.SEED_BASE + 7300 + i, n)
        insts.append((sc, pts, decode(co.msm_best(sc, pts, n, 2))))
    with Device(cfg) as d:
        dev = [(d.put(sc), d.put(pts)) for sc, pts, _ in insts]

        def submit(b):
            sel = dev[per * b:per * b + per]
            return cfg.submit_batch_device([s for s, _ in sel], [p for _, p in sel], [n] * per)

        h0, h1 = submit(0), submit(1)
        r0, r1 = cfg.wait_batch(h0), cfg.wait_batch(h1)
        r2 = cfg.wait_batch(submit(2))
        for got, (_, _, exp) in zip(r0 + r1 + r2, insts):
            assert decode(got) == exp
        for (_, dp), (_, pts, _) in zip(dev, insts):
            assert cfg.to_host(dp, 64 * n) == pts


# ---- 7. partials leave mapped back ----------------------------------------------------------------------------------
def test_gpu_with_cpu_and_range_split(cfg, msm_pkg, pool):
    pts, want = pool
    ks, exp = want[1000]
    sc = mont(ks)
    for split in (1, 500, 999):
        assert decode(msm_pkg.gpu_with_cpu(sc, pts, cfg, split_at=split)) == exp, split
    second = msm_pkg.setup_metal_state(cfg.device())
    try:
        assert decode(msm_pkg.msm_range_multi([cfg, second], sc, pts, 1000)) == exp
    finally:
        second.close()
    assert decode(msm_pkg.msm_best(sc, pts, cfg)) == exp


def test_stage_tap_after_an_in_place_call(cfg, msm_pkg, pool):
    pts, want = pool
    ks, _ = want[1000]
    out = ps._run(cfg, msm_pkg, [(ks, pts)], c=5)[0]
    ps.check_buckets(cfg, msm_pkg, ks, pts, out, 5)   # co.stage_buckets / co.stage_partials on E


# ---- 8. field level, on the device ----------------------------------------------------------------------------------
def test_shifted_unpack_identity_and_negation_device(cfg, msm_pkg):
    host.check_unpack(cfg.test_op_raw)


def test_affine_start_and_mixed_addition_on_the_isomorphic_curve_device(cfg, msm_pkg):
    host.check_additions(cfg.test_op_raw)
