"""The (tile_log, log_n) shapes the GPU transform tests run, in one place: EXISTING restates the sizes of
tests/test_gpu_ntt.py, tests/test_gpu_ntt_geometry.py takes its sizes from here, MANY_WORKGROUPS restates those of
tests/test_gpu_many_workgroups.py, and tests/test_ntt_plan_host.py accounts
on the CPU for the pass geometries these shapes reach (every pass of a shape runs on the GPU, in both directions)."""

DEFAULT_TILE = 10
MAX_LOG = 28

# tests/test_gpu_ntt.py: test_small_sizes, the three-pass size, test_small_tiles
EXISTING = ([(DEFAULT_TILE, log_n) for log_n in range(14)] + [(DEFAULT_TILE, 21)]
            + [(tile_log, log_n) for tile_log in (2, 3) for log_n in range(1, 10)])

# tests/test_gpu_ntt_geometry.py: the two-pass sizes of the default tile
GEOMETRY_DEFAULT = [(DEFAULT_TILE, log_n) for log_n in range(14, 21)]

MID_TILES = tuple(range(4, 10))


def mid_tile_logs(tile_log):
    """one, two and three passes at a tile of 2^tile_log, at least up to 2^16"""
    return range(1, max(16, 2 * tile_log + 1) + 1)


GEOMETRY_TILES = [(tile_log, log_n) for tile_log in MID_TILES for log_n in mid_tile_logs(tile_log)]

# pass taps: (tile_log, log_n)
TAPS = [(DEFAULT_TILE, 12), (DEFAULT_TILE, 16), (DEFAULT_TILE, 20), (DEFAULT_TILE, 21), (3, 7), (6, 13)]

# tests/test_gpu_many_workgroups.py: the three-pass sizes whose middle passes are (8, 2) and (9, 1)
MANY_WORKGROUPS = [(DEFAULT_TILE, 23), (DEFAULT_TILE, 26)]

ALL = EXISTING + GEOMETRY_DEFAULT + GEOMETRY_TILES + MANY_WORKGROUPS


def geometry(passes):
    """the tuples (levels, low, sigma > low, first, last) of a plan as msm_amd_test_ntt_plan returns it: what decides
    the path a pass takes through the kernel"""
    return {(p["levels"], p["low"], p["sigma"] > p["low"], k == 0, k + 1 == len(passes)) for k, p in enumerate(passes)}
