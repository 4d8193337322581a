"""The size thresholds of DESIGN.md's audit table (section 8.20) for the lookup, permute, sort and transform calls, recomputed on
the CPU from the plan aids (msm_amd_test_fr_lookup_plan, msm_amd_test_fr_permute_plan, msm_amd_test_fr_sort_plan,
msm_amd_test_ntt_plan) and compared with the sizes tests/test_gpu_many_workgroups.py runs.  A change of kSortTile,
kPermuteTileLog or kNttTileLog moves a threshold, fails here, and sends its author to the sizes of that file and to the
table."""
import pytest

import lookup_ref as lr
import ntt_shapes as shapes
import permute_ref as pr
import sort_ref as sr


def first(holds, lo, hi):
    """the smallest n in [lo, hi] at which a monotone predicate holds"""
    assert not holds(lo) and holds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if holds(mid) else (mid, hi)
    return hi


def shipped_tile_log(msm_pkg, aid, low):
    """the largest tile_log a plan aid accepts: the aids refuse more than the shipped constant"""
    ok = []
    for tile_log in range(low, 20):
        try:
            aid(tile_log)
            ok.append(tile_log)
        except msm_pkg.MsmError as e:
            assert e.status == msm_pkg.INPUT_ERROR
    assert ok == list(range(low, ok[-1] + 1))
    return ok[-1]


def test_sort(msm_pkg):
    def tiles(n):
        return msm_pkg.test_fr_sort_plan(n, 1, 0xFFFFFFFF)["tiles"]
    assert first(lambda n: tiles(n) >= 2, 1, 1 << 31) == sr.TILE + 1 == 4097                   # a second workgroup of a pass
    # fr_sort_row_scan_kernel: 1024 threads, waves of 64: lane 0 of the second wave holds a count from 65 tiles on ...
    assert first(lambda n: tiles(n) > sr.WAVE, 1, 1 << 31) == sr.N_65_TILES == 262145
    # ... and its loop over the tiles takes a second trip from 1025 tiles on
    assert first(lambda n: tiles(n) > sr.ROW_SCAN_THREADS, 1, 1 << 31) == sr.N_1025_TILES == 4194305
    assert tiles(sr.N_65_TILES) == 65 and tiles(sr.N_1025_TILES) == 1025 and tiles(max(sr.SIZES)) == 4
    assert first(lambda n: tiles(n) > 2 * sr.ROW_SCAN_THREADS, 1, 1 << 31) == 2 * sr.N_1025_TILES - 1   # a third trip: 2^23 + 1, open
    for mask, passes in ((0x3, 2), (0x23, 3), (0, 0), (0xFFFFFFFF, 32)):                      # the masks of the 1025-tile columns
        plan = msm_pkg.test_fr_sort_plan(sr.N_1025_TILES, 1, mask)
        assert plan["passes"] == passes and plan["launches"] == sr.plan(sr.N_1025_TILES, 1, mask)["launches"]
    assert sr.plan(9, 1, 0x23) == dict(passes=3, launches=1 + 2 + 9 + 1, tiles=1)              # bytes 0, 1, 5: two gather words


def test_permute(msm_pkg):
    T = shipped_tile_log(msm_pkg, lambda t: msm_pkg.test_fr_permute_plan(5, 1, t), 2)
    assert T == pr.DEFAULT_TILE_LOG == 11

    def levels(n_rows):
        return msm_pkg.test_fr_permute_plan(n_rows, 1, T)["levels"]
    assert first(lambda n: levels(n) >= 2, 1, (1 << 31) - 1) == (1 << T) + 1 == 2049
    assert first(lambda n: levels(n) >= 3, 1, (1 << 31) - 1) == (1 << 2 * T) + 1 == (1 << 22) + 1   # open: tile knob only
    assert levels((1 << 31) - 1) == 3
    assert [levels(n) for n in pr.SHIPPED_TILE_SIZES] == [1, 1, 2, 2]
    assert pr.SHIPPED_TILE_SIZES[:3] == ((1 << T) - 1, 1 << T, (1 << T) + 1)
    n = pr.SHIPPED_TILE_SIZES[3]
    plan = msm_pkg.test_fr_permute_plan(n, 2, T)
    assert plan["tiles"] == 2 * 33 and n % (1 << T) == 3 and plan == pr.plan(n, 2, T)          # the last tile holds three counters
    assert msm_pkg.test_fr_permute_plan(300, 2, 2)["levels"] == 5                               # what the tile knob reaches on 300 rows


def test_transform(msm_pkg):
    T = shipped_tile_log(msm_pkg, lambda t: msm_pkg.test_ntt_plan(5, t), 2)
    assert T == shapes.DEFAULT_TILE == 10

    def passes(log_n):
        return len(msm_pkg.test_ntt_plan(log_n, T))

    def middle(log_n):
        plan = msm_pkg.test_ntt_plan(log_n, T)
        return {(p["levels"], p["low"]) for p in plan[1:-1]}
    assert [first(lambda x: passes(x) >= k, 0, shapes.MAX_LOG) for k in (2, 3)] == [T + 1, 2 * T + 1]
    assert passes(shapes.MAX_LOG) == 3
    seen = {}
    for log_n in range(shapes.MAX_LOG + 1):
        for geo in middle(log_n):
            seen.setdefault(geo, log_n)
    assert seen == {(7, 3): 21, (8, 2): 23, (9, 1): 26}                                         # the first size of every middle pass
    assert (T, 21) in shapes.EXISTING
    assert [log_n for _, log_n in shapes.MANY_WORKGROUPS] == [seen[(8, 2)], seen[(9, 1)]]
    assert all(tile_log == T for tile_log, _ in shapes.MANY_WORKGROUPS)


def test_lookup(msm_pkg):
    small, large = lr.MANY_ROWS
    assert (-(-small // lr.THREADS), -(-large // lr.THREADS)) == (257, 1024)                    # workgroups of the insert launch
    # the capacity is the power of two >= 2 n_rows: 2^16 + 1 rows sit just above a load of 1/4, 2^18 rows at 1/2 exactly
    assert msm_pkg.test_fr_lookup_plan(small)["capacity"] == 1 << 18 and msm_pkg.test_fr_lookup_plan(small - 1)["capacity"] == 1 << 17
    assert msm_pkg.test_fr_lookup_plan(large)["capacity"] == 1 << 19 and msm_pkg.test_fr_lookup_plan(large + 1)["capacity"] == 1 << 20
    assert msm_pkg.test_fr_lookup_plan(large)["home_bits"] == 19
    chain = msm_pkg.test_fr_lookup_plan(lr.CHAIN_ROWS, lr.CHAIN_BITS)
    assert chain["capacity"] == 1 << 15 and chain["home_bits"] == lr.CHAIN_BITS == 8
    assert lr.CHAIN_ROWS >= 1 << 13 and (1 << lr.CHAIN_BITS) < lr.CHAIN_ROWS // 2               # fewer homes than classes: the run wraps
    with pytest.raises(msm_pkg.MsmError):
        msm_pkg.test_fr_lookup_plan(1 << 31)
