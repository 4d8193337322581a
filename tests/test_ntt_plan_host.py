"""The pass geometry of the transform on the CPU: the plan (ntt_plan, ntt_pass) and the slot map (ntt_slot_index) of
csrc/ntt.hip.h through msm_amd_test_ntt_plan and msm_amd_test_ntt_slots -- the functions the kernel calls, compiled for
the host -- against the properties ntt_pass_kernel relies on; the host twin stopped after some levels
(msm_amd_test_host_ntt_levels) against the integer model of tests/ntt_ref.py; and an account of which pass geometries
the GPU shapes of tests/ntt_shapes.py reach."""
import ctypes
import random

import numpy as np
import pytest

import ntt_ref as m
import ntt_shapes as shapes

R = m.R
TILES = range(2, 11)


def slots_of(msm_pkg, log_n, tile_log, pass_index, wgs):
    """(len(wgs), 2^tile_log) array of flat element indices"""
    L = msm_pkg.lib()
    out = (ctypes.c_uint64 * (1 << tile_log))()
    rows = np.empty((len(wgs), 1 << tile_log), dtype=np.uint64)
    for row, wg in enumerate(wgs):
        assert L.msm_amd_test_ntt_slots(log_n, tile_log, pass_index, wg, out) == msm_pkg.OK
        rows[row] = np.frombuffer(out, dtype=np.uint64)
    return rows


# ---- 1. the model of the network ------------------------------------------------------------------------------------------
def test_all_levels_of_the_model_are_the_transform():
    for log_n in (0, 1, 2, 5, 8):
        n = 1 << log_n
        a = m.random_vector(50 + log_n, n)
        for root in m.ROOTS:
            g = 3 + log_n
            state = m.levels_state(a, root, log_n, m.FORWARD, g, log_n)
            assert [state[m.bitrev(k, log_n)] for k in range(n)] == m.transform(a, root, log_n, m.FORWARD, g)
            assert state == m.levels_state(a, root, log_n, m.FORWARD, g)
            state = m.levels_state(a, root, log_n, m.INVERSE, g, log_n)
            n_inv, g_inv = pow(n, -1, R), pow(g, -1, R)
            got = [state[m.bitrev((n - i) % n, log_n)] * n_inv * pow(g_inv, i, R) % R for i in range(n)]
            assert got == m.transform(a, root, log_n, m.INVERSE, g)
            assert m.levels_state(a, root, log_n, m.INVERSE, g, 0) == a
            assert m.levels_state(a, root, log_n, m.FORWARD, g, 0) == [x * pow(g, i, R) % R for i, x in enumerate(a)]
    assert [m.bitrev(x, 3) for x in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and m.bitrev(0, 0) == 0


# ---- 2. the plan ------------------------------------------------------------------------------------------------------
def test_plan(msm_pkg):
    for tile_log in TILES:
        for log_n in range(shapes.MAX_LOG + 1):
            plan = msm_pkg.test_ntt_plan(log_n, tile_log)
            assert len(plan) == (max(1, -(-log_n // tile_log))), (tile_log, log_n)
            levels = [p["levels"] for p in plan]
            assert sum(levels) == log_n and max(levels) <= tile_log
            assert levels == sorted(levels, reverse=True) and levels[0] - levels[-1] <= 1
            level0 = 0
            for p in plan:
                assert p["level0"] == level0
                assert p["sigma"] == log_n - level0 - p["levels"]
                assert p["low"] == min(p["sigma"], tile_log - p["levels"])
                level0 += p["levels"]


def test_plan_and_slot_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    bad, ok = msm_pkg.INPUT_ERROR, msm_pkg.OK
    plan = (ctypes.c_uint32 * 113)(*([0xA5A5A5A5] * 113))
    slots = (ctypes.c_uint64 * 1024)(*([0xA5] * 1024))
    assert L.msm_amd_test_ntt_plan(29, 10, plan) == bad and L.msm_amd_test_ntt_plan(5, 1, plan) == bad
    assert L.msm_amd_test_ntt_plan(5, 11, plan) == bad and L.msm_amd_test_ntt_plan(5, 10, None) == bad
    assert L.msm_amd_test_ntt_slots(29, 10, 0, 0, slots) == bad and L.msm_amd_test_ntt_slots(5, 1, 0, 0, slots) == bad
    assert L.msm_amd_test_ntt_slots(5, 11, 0, 0, slots) == bad and L.msm_amd_test_ntt_slots(5, 10, 0, 0, None) == bad
    assert L.msm_amd_test_ntt_slots(5, 10, 1, 0, slots) == bad               # one pass: no pass 1
    assert L.msm_amd_test_ntt_slots(21, 10, 3, 0, slots) == bad              # three passes
    assert L.msm_amd_test_ntt_slots(5, 10, 0, 1 << 32, slots) == bad         # a grid has fewer than 2^32 workgroups
    assert all(v == 0xA5A5A5A5 for v in plan) and all(v == 0xA5 for v in slots)
    assert L.msm_amd_test_ntt_plan(28, 2, plan) == ok and plan[0] == 14 and plan[112] == 0xA5A5A5A5
    assert L.msm_amd_test_ntt_slots(21, 10, 2, 5, slots) == ok

    data = m.encode(list(range(8)), m.CANON_LE)
    out = ctypes.create_string_buffer(b"\xA5" * 256, 256)

    def levels(root=0, log_n=3, direction=0, layout=1, shift=None, src=data, dst=out, n_vec=1, count=2):
        return L.msm_amd_test_host_ntt_levels(root, log_n, direction, layout, shift, src, dst, n_vec, count, 1)

    assert levels(root=2) == bad and levels(direction=2) == bad and levels(layout=msm_pkg.SCALAR_CANON_BE32) == bad
    assert levels(count=4) == bad and levels(count=0xFFFFFFFF) == bad and levels(log_n=29, n_vec=0) == bad
    assert levels(src=None) == bad and levels(dst=None) == bad and levels(shift=bytes(32)) == bad
    assert levels(n_vec=1 << 29) == bad
    assert levels(n_vec=0) == ok and levels(n_vec=0, src=None, dst=None) == ok
    assert out.raw == b"\xA5" * 256
    assert levels(count=3) == ok and out.raw[:256] != b"\xA5" * 256


# ---- 3. the slot map ----------------------------------------------------------------------------------------------------
def gb_of(p, b):
    """the element bit a slot bit stands for, from the head comment of ntt.hip.h: slot bits [0, low) are the low index
    bits, [low, low + t) the position in the tile, which sits at stride 2^sigma, and bits from low + t on -- they exist
    only when low = sigma -- count further tiles, above the tile bits"""
    if b < p["low"]:
        return b
    if b < p["low"] + p["levels"]:
        return p["sigma"] + (b - p["low"])
    assert p["low"] == p["sigma"]
    return b


@pytest.mark.parametrize("tile_log", TILES)
def test_slot_map(msm_pkg, tile_log):
    size = 1 << tile_log
    for log_n in range(15):
        n = 1 << log_n
        plan = msm_pkg.test_ntt_plan(log_n, tile_log)
        for n_vec in (1, 3):
            total = n_vec * n
            wgs = -(-total // size)
            for k, p in enumerate(plan):
                where = (tile_log, log_n, n_vec, k)
                idx = slots_of(msm_pkg, log_n, tile_log, k, range(wgs))
                flat = idx.reshape(-1)
                assert np.array_equal(np.sort(flat), np.arange(wgs * size, dtype=np.uint64)), where    # a bijection
                assert np.all(idx[:, 1:] > idx[:, :-1]), where                # the write-back's break
                wg_of = np.empty(wgs * size, dtype=np.int64)
                slot_of = np.empty(wgs * size, dtype=np.int64)
                wg_of[flat.astype(np.int64)] = np.repeat(np.arange(wgs), size)
                slot_of[flat.astype(np.int64)] = np.tile(np.arange(size), wgs)
                elems = np.arange(total, dtype=np.int64)
                for level in range(p["level0"], p["level0"] + p["levels"]):
                    h = n >> (level + 1)
                    i = elems[(elems & h) == 0]
                    assert np.array_equal(wg_of[i], wg_of[i + h]), (where, level)
                    bit = p["low"] + p["levels"] - 1 - (level - p["level0"])     # the kernel's pb
                    assert np.all(slot_of[i] ^ slot_of[i + h] == 1 << bit), (where, level)
                    assert np.all(slot_of[i] & (1 << bit) == 0), (where, level)
                for b in (8, 9):      # the stepping of the powers of g: a thread's slots are tid + 256 r
                    if b < tile_log:
                        lower = (np.arange(size) >> b) & 1 == 0
                        step = idx[:, np.flatnonzero(lower) | (1 << b)] - idx[:, lower]
                        assert np.all(step == 1 << gb_of(p, b)), (where, b)


def test_slot_map_in_64_bits(msm_pkg):
    """the largest call: 2^28 elements, 15 vectors -- flat indices up to 15 * 2^28 > 2^31"""
    log_n, tile_log, n_vec = 28, 10, 15
    total = n_vec << log_n
    wgs = total >> tile_log
    picked = [0, wgs - 1] + random.Random(64).sample(range(1, wgs - 1), 64)
    plan = msm_pkg.test_ntt_plan(log_n, tile_log)
    assert [p["levels"] for p in plan] == [10, 9, 9]
    for k, p in enumerate(plan):
        t, sigma, low = p["levels"], p["sigma"], p["low"]
        idx = slots_of(msm_pkg, log_n, tile_log, k, picked)
        # the bit permutation, written out: c = wg 2^T + m.  Index bit j is
        #   c_j for j < low; c_(j + t) for low <= j < sigma (the tile number continues past the position bits);
        #   c_(low + j - sigma) for sigma <= j < sigma + t (the position in the tile); c_j above.
        c = (np.array(picked, dtype=np.uint64)[:, None] << np.uint64(tile_log)) | np.arange(1 << tile_log, dtype=np.uint64)[None, :]
        exp = np.zeros_like(c)
        for j in range(40):
            src = j if j < low else j + t if j < sigma else low + j - sigma if j < sigma + t else j
            exp |= ((c >> np.uint64(src)) & np.uint64(1)) << np.uint64(j)
        assert np.array_equal(idx, exp), k
        assert int(idx.max()) < total, k


# ---- 4. which geometries the GPU shapes reach -----------------------------------------------------------------------------
def reached(msm_pkg, tile_log, shape_list):
    out = set()
    for tl, log_n in shape_list:
        if tl == tile_log:
            out |= shapes.geometry(msm_pkg.test_ntt_plan(log_n, tile_log))
    return out


def test_gpu_shapes_cover_the_geometries(msm_pkg):
    T = shapes.DEFAULT_TILE
    possible = set()
    first_seen = {}
    for log_n in range(shapes.MAX_LOG + 1):
        for geo in shapes.geometry(msm_pkg.test_ntt_plan(log_n, T)):
            first_seen.setdefault(geo, log_n)
            possible.add(geo)
    assert len(possible) == 25
    before = reached(msm_pkg, T, shapes.EXISTING)
    assert len(possible - before) == 8 and all(geo[0] >= 8 for geo in possible - before)
    # (levels, low, sigma > low, first, last): the middle passes from 2^23 and from 2^26 on, which differ from the first passes
    # of 2^15, 2^16 and 2^17, 2^18 only in `first` (ntt_load and the FORWARD shift); tests/test_gpu_many_workgroups.py runs them
    large = {(8, 2, True, False, False), (9, 1, True, False, False)}
    assert possible - reached(msm_pkg, T, shapes.ALL) == set()
    assert possible - reached(msm_pkg, T, shapes.EXISTING + shapes.GEOMETRY_DEFAULT + shapes.GEOMETRY_TILES) == large
    assert large <= reached(msm_pkg, T, shapes.MANY_WORKGROUPS)
    assert first_seen[(8, 2, True, False, False)] == 23 and first_seen[(9, 1, True, False, False)] == 26
    assert {(8, 2, True, True, False), (9, 1, True, True, False)} <= reached(msm_pkg, T, shapes.GEOMETRY_DEFAULT)
    for tile_log in shapes.MID_TILES:
        counts = {}
        for tl, log_n in shapes.ALL:
            if tl == tile_log:
                counts.setdefault(len(msm_pkg.test_ntt_plan(log_n, tile_log)), log_n)
        assert {1, 2, 3} <= set(counts), tile_log
        middle = {geo for geo in reached(msm_pkg, tile_log, shapes.ALL) if not geo[3] and not geo[4]}
        assert middle, tile_log
    for tile_log, log_n in shapes.TAPS:
        assert (tile_log, log_n) in shapes.ALL
        assert len(msm_pkg.test_ntt_plan(log_n, tile_log)) >= 2


# ---- 5. the twin, level by level ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(14))
def test_host_levels_against_the_model(msm_pkg, log_n):
    n = 1 << log_n
    a = m.random_vector(1300 + log_n, n)
    root = log_n & 1
    g = random.Random(1300 + log_n).randrange(2, R)
    for direction in m.DIRECTIONS:
        for shift in (None, g):
            layout = (log_n + direction + (shift is None)) & 1
            data, rec = m.encode(a, layout), m.shift_record(shift, layout)
            for levels, state in enumerate(m.level_states(a, root, log_n, direction, shift or 1)):
                got = msm_pkg.test_host_ntt_levels(data, root, log_n, levels, direction, layout, rec)
                assert got == m.encode(state, m.MONT_LE), (direction, shift is None, levels)
    assert m.levels_state(a, root, log_n, m.FORWARD, g, log_n // 2) == \
        m.decode(msm_pkg.test_host_ntt_levels(m.encode(a, m.CANON_LE), root, log_n, log_n // 2, m.FORWARD, m.CANON_LE,
                                              m.shift_record(g, m.CANON_LE)), m.MONT_LE)


def test_host_levels_of_a_batch(msm_pkg):
    log_n, n_vec = 6, 3
    n = 1 << log_n
    a = m.random_vector(66, n_vec * n)
    for levels in range(log_n + 1):
        exp = [x for v in range(n_vec) for x in m.levels_state(a[v * n:(v + 1) * n], m.H2C, log_n, m.FORWARD, 9, levels)]
        got = msm_pkg.test_host_ntt_levels(m.encode(a, m.MONT_LE), m.H2C, log_n, levels, m.FORWARD, m.MONT_LE,
                                           m.shift_record(9, m.MONT_LE), n_vec, threads=3)
        assert got == m.encode(exp, m.MONT_LE), levels
