"""The lookup, permute, sort and transform calls at sizes that take many workgroups at the SHIPPED geometry (the
audit table of section 8.20).  The other GPU tests of these families shrink the geometry with an env knob and stay at a few
thousand records; here the sizes are the ones at which the shipped constants start a new path -- an index built by hundreds
of workgroups at once, the second scan level of the permute at kPermuteTileLog = 11, the row scan of the sort past one wave
(65 tiles) and past one trip (1025 tiles), the middle passes (8, 2) and (9, 1) of the transform, and two thresholds the audit
found beside them (the running sums and the term-list sumcheck round at three levels) -- and the references are
the big-integer models where they are fast enough, the numpy models of the *_ref modules (pinned to the big-integer models by
tests/test_np_models_host.py) and the host twins (pinned to the models by the *_host tests) beyond.  Every comparison is of
bytes.  Every call here is a valid call; nothing here tries to make a kernel fail."""
import ctypes
import functools
import random

import numpy as np
import pytest

import lookup_ref as lr
import ntt_ref as m
import ntt_shapes as shapes
import permute_halo2_ref as hr
import permute_ref as pr
import sort_ref as sr
import terms_ref as t

pytestmark = pytest.mark.gpu

R = lr.R
FF = b"\xFF"
DEVICE = sr.MEM_DEVICE


class Device:
    """device buffers of one test, freed together"""

    def __init__(self, cfg):
        self.cfg, self.ptrs = cfg, []

    def alloc(self, nbytes, fill=None):
        d = self.cfg.alloc(max(32, nbytes))
        self.ptrs.append(d)
        if fill is not None:
            self.cfg.to_device(d, fill * nbytes)
        return d

    def put(self, data):
        d = self.alloc(len(data))
        self.cfg.to_device(d, data)
        return d

    def words(self, d, count):
        return np.frombuffer(self.cfg.to_host(d, 4 * count), dtype=np.uint32)

    def records(self, d, count):
        return np.frombuffer(self.cfg.to_host(d, 32 * count), dtype=np.uint32).reshape(-1, 8)

    def close(self):
        for d in self.ptrs:
            self.cfg.free(d)
        self.ptrs = []


@pytest.fixture
def dev(cfg):
    d = Device(cfg)
    yield d
    d.close()


def same_records(got, exp, tag):
    """two (n, 8) uint32 arrays, or bytes; names the first record that differs"""
    got = np.frombuffer(got, dtype=np.uint32).reshape(-1, 8) if isinstance(got, bytes) else got
    exp = np.frombuffer(exp, dtype=np.uint32).reshape(-1, 8) if isinstance(exp, bytes) else exp
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (tag, "%d records differ, the first is %d" % (bad.size, bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())


def same_words(got, exp, tag):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (tag, "%d words differ, the first is %d" % (bad.size, bad[0]), int(got[bad[0]]), int(exp[bad[0]]))


# ==== 1. lookup: an index built by hundreds of workgroups ==========================================================================
@functools.lru_cache(maxsize=None)
def spread_case(n_rows, layout, r_class_rows=None):
    """(table records, (n_rows, 8) array of them, rep_of_row as int64, the rows of the class of 1024) of lr.spread_table; the
    representatives are those of the big-integer model"""
    words, many = lr.spread_table(n_rows + layout, n_rows, r_class_rows)
    table = lr.raw(words)
    rep = lr.representatives(table, layout)
    rep_of_row = np.array([rep[v] for v in lr.decode(table, layout)], dtype=np.int64)
    assert lr.n_distinct(table, layout) == len(rep) == np.unique(rep_of_row).size
    return table, sr.np_from_bytes(table), rep_of_row, many


def both_builds(cfg, dev, table, layout):
    """a handle built from host rows and one built from device rows, which are overwritten afterwards"""
    d_table = dev.put(table)
    hs = [cfg.fr_lookup_build(table, layout)]
    try:
        hs.append(cfg.fr_lookup_build_device(d_table, len(table) // 32, layout))
    except Exception:
        hs[0].free()
        raise
    cfg.to_device(d_table, b"\xEE" * len(table))
    return hs


def check_index(cfg, msm_pkg, dev, h, table, layout, rep_of_row, hash_bits, tag):
    """the handle's statistics and its image against the model, then a probe of every row's own value.  Returns
    (n_distinct, longest_probe, the slot words)."""
    n_rows = len(table) // 32
    info, plan = h.info(), msm_pkg.test_fr_lookup_plan(n_rows, hash_bits)
    cap = plan["capacity"]
    assert info["n_rows"] == n_rows and info["capacity"] == cap and info["device_bytes"] == plan["bytes"], tag
    distinct = int(np.unique(rep_of_row).size)
    assert info["n_distinct"] == distinct, tag
    image = cfg.test_fr_lookup_image(h)
    rows = np.frombuffer(cfg.to_host(image, 32 * n_rows), dtype=np.uint32).reshape(-1, 8)
    slots = np.frombuffer(cfg.to_host(image + plan["slots_off"], 4 * cap), dtype=np.uint32)
    stats = np.frombuffer(cfg.to_host(image + plan["slots_off"] + 4 * cap, 32), dtype=np.uint32)
    assert lr.decode(rows.tobytes(), lr.MONT_LE) == lr.decode(table, layout), tag          # reduced Montgomery residues
    assert rows.tobytes() == lr.encode(lr.decode(rows.tobytes(), lr.MONT_LE), lr.MONT_LE), tag
    classes, longest = lr.check_slots(slots, rows, rep_of_row, plan["home_bits"])
    assert classes == distinct, tag
    assert stats.tolist() == [distinct, longest, 0, 0, 0, 0, 0, 0], (tag, stats.tolist(), longest)   # kLookupDistinct, Longest, Error
    assert info["longest_probe"] == longest, tag
    d_in = dev.put(table)
    d_m, d_idx = dev.alloc(32 * n_rows, FF), dev.alloc(4 * n_rows, FF)
    rep, _ = cfg.fr_lookup_multiplicities_device(h, d_in, n_rows, d_m, d_idx, msm_pkg.LOOKUP_STRICT, layout)
    counts = np.bincount(rep_of_row, minlength=n_rows)
    assert rep == dict(n_missing=0, first_missing=lr.NO_MISS, rows_hit=distinct, max_multiplicity=int(counts.max())), (tag, rep)
    same_words(dev.words(d_idx, n_rows), rep_of_row, (tag, "idx"))
    same_records(dev.records(d_m, n_rows), lr.encode(counts.tolist(), layout), (tag, "m"))
    assert cfg.to_host(d_in, len(table)) == table, tag
    return distinct, longest, slots


@pytest.mark.parametrize("layout", lr.LAYOUTS)
@pytest.mark.parametrize("n_rows", lr.MANY_ROWS)
def test_lookup_duplicates_across_workgroups(cfg, msm_pkg, dev, n_rows, layout):
    """257 and 1024 workgroups insert at once.  The members of a class sit n_rows / 2 >= 2^15 rows apart, so they arrive from
    different workgroups, in whatever order the hardware runs them (a test cannot choose that order; a class of three has
    its smallest index in the first workgroup, its largest in the last); the class of 1024 races for one slot from 1024
    places; one class stands under the words v, v + r, v + 2r."""
    table, _, rep_of_row, many = spread_case(n_rows, layout)
    assert abs(np.unique(rep_of_row).size - n_rows // 2) < 1100 and (rep_of_row[many] == 17).all()
    assert rep_of_row[0] == rep_of_row[n_rows // 2] == rep_of_row[n_rows - 1] == 0
    hs = both_builds(cfg, dev, table, layout)
    try:
        for k, h in enumerate(hs):
            check_index(cfg, msm_pkg, dev, h, table, layout, rep_of_row, 32, (n_rows, layout, k))
    finally:
        for h in hs:
            h.free()


N_INPUTS, N_COLS = 1 << 18, 2
ROW_OF_HALF = 40000


@functools.lru_cache(maxsize=None)
def picks(kind):
    """the row every input is drawn from: the distributions of tools/lookup_bench.py"""
    n_rows = lr.MANY_ROWS[0]
    rng = np.random.default_rng(len(kind))
    if kind == "uniform":
        return rng.integers(0, n_rows, N_INPUTS)
    if kind == "half one row":
        return np.where(np.arange(N_INPUTS) & 1, ROW_OF_HALF, rng.integers(0, n_rows, N_INPUTS))
    assert kind == "all one row"
    return np.full(N_INPUTS, n_rows - 1)


@pytest.mark.parametrize("layout", lr.LAYOUTS)
@pytest.mark.parametrize("count", ["block", "wave", "lane"])
def test_lookup_multiplicities(cfg, msm_pkg, dev, count, layout, monkeypatch):
    """2^18 inputs in two columns over the table of 2^16 + 1 rows: 256 workgroups of 16 waves (block) or 1024 of 4 add to the
    same counters.  An input is a copy of the record of a row, so the model is lookup_ref.np_multiplicities over the classes
    of the rows, a class being named by its representative from the big-integer model.  Then one STRICT call with a miss in the first and one in the last workgroup."""
    monkeypatch.setenv("MSM_AMD_LOOKUP_COUNT", count)
    n_rows = lr.MANY_ROWS[0]
    table, rec, rep_of_row, _ = spread_case(n_rows, layout)
    h = cfg.fr_lookup_build(table, layout)
    try:
        d_in = dev.alloc(32 * N_INPUTS)
        d_m, d_idx = dev.alloc(32 * n_rows), dev.alloc(4 * N_INPUTS)
        for kind in ("uniform", "half one row", "all one row"):
            pick = picks(kind)
            counts, idx, exp_rep = lr.np_multiplicities(rep_of_row, rep_of_row[pick])
            assert exp_rep["n_missing"] == 0 and exp_rep["max_multiplicity"] >= (1 if kind == "uniform" else N_INPUTS // 2)
            data = rec[pick].tobytes()
            cfg.to_device(d_in, data)
            cfg.to_device(d_m, FF * (32 * n_rows))
            cfg.to_device(d_idx, FF * (4 * N_INPUTS))
            rep, _ = cfg.fr_lookup_multiplicities_device(h, d_in, N_INPUTS // N_COLS, d_m, d_idx, msm_pkg.LOOKUP_COUNT_MISSING,
                                                         layout, N_COLS)
            assert rep == exp_rep, (kind, rep, exp_rep)
            same_words(dev.words(d_idx, N_INPUTS), idx, (kind, "idx"))
            same_records(dev.records(d_m, n_rows), lr.encode(counts.tolist(), layout), (kind, "m"))
            assert cfg.to_host(d_in, len(data)) == data, kind
        # STRICT: misses in the first and in the last workgroup; m_out stays as it was
        pick = picks("uniform")
        missing = (3, N_INPUTS - 2)
        absent = lr.raw([0xABCDEF, 0xABCDF0])
        assert not set(lr.decode(absent, layout)) & set(lr.decode(table, layout))
        raw = bytearray(rec[pick].tobytes())
        for k, i in enumerate(missing):
            raw[32 * i:32 * i + 32] = absent[32 * k:32 * k + 32]
        classes = rep_of_row[pick]
        classes[list(missing)] = n_rows                          # the class of no row
        _, idx, exp_rep = lr.np_multiplicities(rep_of_row, classes)
        assert (exp_rep["n_missing"], exp_rep["first_missing"]) == (2, 3) and (idx[list(missing)] == lr.NOT_FOUND).all()
        cfg.to_device(d_in, bytes(raw))
        cfg.to_device(d_m, FF * (32 * n_rows))
        cfg.to_device(d_idx, FF * (4 * N_INPUTS))
        with pytest.raises(msm_pkg.MsmError) as e:
            cfg.fr_lookup_multiplicities_device(h, d_in, N_INPUTS // N_COLS, d_m, d_idx, msm_pkg.LOOKUP_STRICT, layout, N_COLS)
        assert e.value.status == msm_pkg.INPUT_ERROR and e.value.report == exp_rep, (e.value, e.value.report, exp_rep)
        assert cfg.to_host(d_m, 32 * n_rows) == FF * (32 * n_rows)
        same_words(dev.words(d_idx, N_INPUTS), idx, "strict idx")
    finally:
        h.free()


CHAIN_BITS, CHAIN_ROWS = lr.CHAIN_BITS, lr.CHAIN_ROWS


@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_lookup_long_chains_across_the_end(cfg, msm_pkg, dev, layout, monkeypatch):
    """MSM_AMD_LOOKUP_HASH_BITS = 8 on 12 289 rows (6 144 rows, repeated 6 144 rows on, with the classes of spread_table): 256
    homes at the top of 32 768 slots serve 6 145 classes, so the chains merge into one run of slots that starts below
    the last slot and wraps to slot 0, and an insert looks at thousands of slots while 49 workgroups fill them.  The host
    twin's build, which is the same probe algorithm, takes 0.07 s at this pair on the development host (one thread, measured
    with the multiplicities twin on one input).  kLookupLongest is the longest walk from a home to its class's slot in the
    image that was built (check_slots); it is at least classes / 256, and no order of arrival can make it exceed the
    classes."""
    monkeypatch.setenv("MSM_AMD_LOOKUP_HASH_BITS", str(CHAIN_BITS))
    half = CHAIN_ROWS // 2
    table, _, rep_of_row, many = spread_case(CHAIN_ROWS, layout, (0, half, CHAIN_ROWS - 1))
    hs = both_builds(cfg, dev, table, layout)
    try:
        for k, h in enumerate(hs):
            distinct, longest, slots = check_index(cfg, msm_pkg, dev, h, table, layout, rep_of_row, CHAIN_BITS, (layout, k))
            assert -(-distinct // (1 << CHAIN_BITS)) <= longest <= distinct
            used = np.flatnonzero(slots != lr.NOT_FOUND)         # one run of slots from a home to the end, and on from slot 0
            assert slots.size == 1 << 15 and used[0] == 0 and used[-1] == slots.size - 1
            gap = np.flatnonzero(np.diff(used) != 1)
            assert gap.size == 1 and used[gap[0] + 1] >= slots.size - (1 << CHAIN_BITS)
        twin = msm_pkg.host_fr_lookup_multiplicities(table, table, msm_pkg.LOOKUP_STRICT, layout, threads=1)
        same_words(np.array(twin[1]), rep_of_row, "twin idx")
    finally:
        for h in hs:
            h.free()


# ==== 2. permute: the levels of the shipped tile ===================================================================================
PAIRS = {"half, uniform": ("half", "uniform"), "shuffle, one row": ("shuffle", "row-1")}


@functools.lru_cache(maxsize=None)
def permute_case(n_rows, pair):
    """(layout, table, two columns, the model's rows order, the model's halo2 order)"""
    layout = (n_rows + len(pair)) & 1
    table = lr.random_table(n_rows, n_rows, layout, distinct=n_rows - n_rows // 4)
    kinds = [k if k != "row-1" else "row%d" % (n_rows - 1) for k in PAIRS[pair]]
    data = b"".join(pr.column(kind, n_rows + k, table, layout, n_rows) for k, kind in enumerate(kinds))
    return layout, table, data, pr.permute(table, data, layout, 2), hr.permute(table, data, layout, 2)


def device_permute(cfg, dev, h, data, how, layout, n, n_vec, want_s=True):
    d_in, d_a = dev.put(data), dev.alloc(len(data), FF)
    d_s = dev.alloc(len(data), FF)
    rep = cfg.fr_lookup_permute_as(h, d_in, how, layout, n_vec, DEVICE, n=n, a_out=d_a, s_out=d_s if want_s else None)[2]
    assert cfg.to_host(d_in, len(data)) == data
    return cfg.to_host(d_a, len(data)), cfg.to_host(d_s, len(data)), rep


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("n_rows,fill", [(n, None) for n in pr.SHIPPED_TILE_SIZES[:3]]
                         + [(pr.SHIPPED_TILE_SIZES[3], fill) for fill in ("search", "scan")])
def test_permute_at_the_shipped_tile(cfg, msm_pkg, dev, n_rows, fill, pair, monkeypatch):
    """n = n_rows round the tile of 2^11 counters (one level up to 2048, two from 2049 on) and at 2^16 + 3 (33 tiles a column,
    the last one of three counters), two columns, so that a column boundary falls inside a tile, a wave and a workgroup of
    the probe: rows order through both calls, halo2 order over a sorted handle, host and device forms, A', S' and the report."""
    if fill:
        monkeypatch.setenv("MSM_AMD_PERMUTE_FILL", fill)
    monkeypatch.delenv("MSM_AMD_PERMUTE_TILE_LOG", raising=False)
    plan = msm_pkg.test_fr_permute_plan(n_rows, 2)
    assert plan["levels"] == (1 if n_rows <= 2048 else 2) and plan["tiles"] == 2 * -(-n_rows // 2048)
    layout, table, data, rows_exp, halo2_exp = permute_case(n_rows, pair)
    assert rows_exp[2] == halo2_exp[2] and rows_exp[2]["n_missing"] == 0 and rows_exp[2]["rows_hit"] > 0
    h = cfg.fr_lookup_build(table, layout)
    hs = None
    try:
        hs, _ = cfg.fr_lookup_build_sorted(table, layout, want_perm=False)
        got = cfg.fr_lookup_permute(h, data, layout, 2)
        same_records(got[0], rows_exp[0], "rows A'"), same_records(got[1], rows_exp[1], "rows S'")
        assert got[2] == rows_exp[2], (got[2], rows_exp[2])
        for name, handle, how, exp in (("rows", h, hr.ROWS, rows_exp), ("halo2", hs, hr.HALO2, halo2_exp)):
            got = cfg.fr_lookup_permute_as(handle, data, how, layout, 2)
            same_records(got[0], exp[0], name + " host A'"), same_records(got[1], exp[1], name + " host S'")
            assert got[2] == exp[2], (name, got[2], exp[2])
            got = device_permute(cfg, dev, handle, data, how, layout, n_rows, 2)
            same_records(got[0], exp[0], name + " device A'"), same_records(got[1], exp[1], name + " device S'")
            assert got[2] == exp[2], (name, got[2], exp[2])
    finally:
        h.free()
        if hs is not None:
            hs.free()


def test_permute_a_alone_with_other_n(cfg, msm_pkg, dev):
    """A' alone, n != n_rows: 7000 inputs a column over 5000 rows (two levels, three tiles a column, so that the rows of two
    tiles start from a total of the level above), both orders, host and device forms"""
    n_rows, n, layout = 5000, 7000, pr.MONT_LE
    table = lr.random_table(77, n_rows, layout, distinct=n_rows - 300)
    assert msm_pkg.test_fr_permute_plan(n_rows, 2)["levels"] == 2
    data = pr.column("half", 1, table, layout, n) + pr.column("uniform", 2, table, layout, n)
    rows_exp, halo2_exp = pr.permute(table, data, layout, 2, want_s=False), hr.permute(table, data, layout, 2, want_s=False)
    h = cfg.fr_lookup_build(table, layout)
    hs = None
    try:
        hs, _ = cfg.fr_lookup_build_sorted(table, layout, want_perm=False)
        assert cfg.fr_lookup_permute(h, data, layout, 2, want_s=False) == rows_exp
        for handle, how, exp in ((h, hr.ROWS, rows_exp), (hs, hr.HALO2, halo2_exp)):
            assert cfg.fr_lookup_permute_as(handle, data, how, layout, 2, want_s=False) == exp, how
            a, s, rep = device_permute(cfg, dev, handle, data, how, layout, n, 2, want_s=False)
            assert (a, rep) == (exp[0], exp[2]) and s == FF * len(data), how
    finally:
        h.free()
        if hs is not None:
            hs.free()


# ==== 3. sort: the row scan past one wave (65 tiles) and past one trip (1025 tiles) ===============================================
def stale_histograms(cfg, dev):
    """a small sort on the same ctx, so that the histograms and the pairs of the next call start stale"""
    rec = sr.np_records(np.random.default_rng(5).integers(0, 1 << 63, 5000, dtype=np.uint64))
    d_in, d_out = dev.put(rec.tobytes()), dev.alloc(32 * 5000)
    cfg.fr_sort(d_in, sr.CANON_LE, 1, DEVICE, n=5000, out=d_out)
    same_records(dev.records(d_out, 5000), sr.np_sort(rec)[0], "the small sort")


def device_sort(cfg, dev, data, layout, n, n_vec):
    """MEM_DEVICE into buffers that start as 0xFF: ((n_vec n, 8) records, uint32 perm)"""
    d_in = dev.put(data)
    d_out, d_perm = dev.alloc(len(data), FF), dev.alloc(4 * n * n_vec, FF)
    cfg.fr_sort(d_in, layout, n_vec, DEVICE, n=n, out=d_out, perm_out=d_perm)
    assert cfg.to_host(d_in, len(data)) == data
    return dev.records(d_out, n * n_vec), dev.words(d_perm, n * n_vec)


N_65_TILES = sr.N_65_TILES                       # 262 145: the 65th tile holds one pair


@pytest.mark.parametrize("layout", sr.LAYOUTS)
def test_sort_65_tiles(cfg, msm_pkg, dev, layout):
    """65 tiles: lane 0 of the second wave of fr_sort_row_scan_kernel holds a count, so the cross-wave half of block_scan
    carries weight.  Full-width random keys (32 passes), two columns; the host twin at every record, the big-integer model
    on the second column of CANON_LE."""
    n, n_vec = N_65_TILES, 2
    assert msm_pkg.test_fr_sort_plan(n, n_vec, 0xFFFFFFFF)["tiles"] == 65
    stale_histograms(cfg, dev)
    rec = m.np_random_records(65 + layout, n * n_vec)
    data = rec.tobytes()
    out = ctypes.create_string_buffer(len(data))
    perm = (ctypes.c_uint32 * (n * n_vec))()
    msm_pkg.host_fr_sort(data, layout, n_vec, n=n, out=out, perm_out=perm)
    got_out, got_perm = device_sort(cfg, dev, data, layout, n, n_vec)
    same_words(got_perm, np.frombuffer(perm, dtype=np.uint32), "perm")
    same_records(got_out, out.raw, "out")
    if layout == sr.CANON_LE:
        exp_out, exp_perm = sr.sort(data[32 * n:], layout)
        assert got_out[n:].tobytes() == exp_out and got_perm[n:].tolist() == exp_perm


def test_sort_65_tiles_is_stable(cfg, msm_pkg, dev):
    """five values over 262 145 records, two columns: runs of ~52 000 equal keys cross every tile; perm ascends inside a run"""
    n, n_vec = N_65_TILES, 2
    pool = np.array([3, (1 << 64) - 1, 1 << 40, 0x0102030405060708, 77 << 8], dtype=np.uint64)
    rec = sr.np_records(pool[np.random.default_rng(6).integers(0, 5, n * n_vec)])
    stale_histograms(cfg, dev)
    got_out, got_perm = device_sort(cfg, dev, rec.tobytes(), sr.CANON_LE, n, n_vec)
    sr.np_runs_ascend(rec, got_perm, n_vec)
    exp_out, exp_perm = sr.np_sort(rec, n_vec)
    same_words(got_perm, exp_perm, "perm"), same_records(got_out, exp_out, "out")


N_1025_TILES = sr.N_1025_TILES                   # 4 194 305: the row scan takes a second trip for one tile of one pair


def columns_1025(kind):
    rng = np.random.default_rng(1025)
    n = N_1025_TILES
    if kind == "below 2^16":
        return rng.integers(0, 1 << 16, n, dtype=np.uint64), 0x3
    if kind == "bytes 0, 1 and 5":
        return rng.integers(0, 1 << 16, n, dtype=np.uint64) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(40)), 0x23
    assert kind == "all equal"
    return np.full(n, 0x1234567890, dtype=np.uint64), 0


@pytest.mark.parametrize("kind", ["below 2^16", "bytes 0, 1 and 5", "all equal"])
def test_sort_1025_tiles(cfg, msm_pkg, dev, kind):
    """1025 tiles: the loop of fr_sort_row_scan_kernel over 1024 tiles at a time takes its second trip, and what it adds there is
    `carry`.  CANON_LE keys below 2^64 against the numpy model: two passes of one gather word, three passes of two gather
    words, and no pass at all (mask 0: perm is the identity)."""
    n = N_1025_TILES
    vals, mask = columns_1025(kind)
    rec = sr.np_records(vals)
    assert sr.np_digit_mask(rec) == mask
    got, exp = msm_pkg.test_fr_sort_plan(n, 1, mask), sr.plan(n, 1, mask)
    assert {k: got[k] for k in exp} == exp and exp["tiles"] == 1025
    stale_histograms(cfg, dev)
    got_out, got_perm = device_sort(cfg, dev, rec.tobytes(), sr.CANON_LE, n, 1)
    exp_out, exp_perm = sr.np_sort(rec)
    same_words(got_perm, exp_perm, "perm"), same_records(got_out, exp_out, "out")
    if not mask:
        assert np.array_equal(got_perm, np.arange(n, dtype=np.uint32))


# ==== 4. transform: the middle passes (8, 2) from 2^23 on and (9, 1) from 2^26 on ================================================
def middle_pass(msm_pkg, log_n):
    plan = msm_pkg.test_ntt_plan(log_n)
    assert len(plan) == 3
    return [p["levels"] for p in plan], (plan[1]["levels"], plan[1]["low"])


def test_ntt_2_23(cfg, msm_pkg, dev):
    """2^23: passes of 8, 8 and 7 levels, the middle one (t = 8, low = 2).  Dense reduced MONT_LE records, device-resident, out
    of place, a shift, every output record against the host twin in both directions; the inverse of the forward output, in
    place, gives the input back."""
    log_n, root, layout = shapes.MANY_WORKGROUPS[0][1], m.H2C, m.MONT_LE
    n = 1 << log_n
    assert middle_pass(msm_pkg, log_n) == ([8, 8, 7], (8, 2))
    data = m.np_random_records(23, n).tobytes()
    shift = m.shift_record(random.Random(23).randrange(2, R), layout)
    dom = cfg.ntt_domain(root, log_n)
    try:
        d_in, d_out = dev.put(data), dev.alloc(32 * n, FF)
        for direction in m.DIRECTIONS:
            exp = msm_pkg.host_ntt(data, root, log_n, direction, layout, shift)
            cfg.ntt_device(dom, d_in, d_out, direction, layout, shift)
            same_records(cfg.to_host(d_out, 32 * n), exp, direction)
            del exp
            if direction == m.FORWARD:
                cfg.ntt_device(dom, d_out, d_out, m.INVERSE, layout, shift)
                same_records(cfg.to_host(d_out, 32 * n), data, "round trip")
        assert cfg.to_host(d_in, 32 * n) == data
    finally:
        dom.free()


CHUNK_LOG = 22                                   # records per copy of the 2^26 vector: 128 MiB


def read_chunks(msm_pkg, cfg, d, log_n):
    """the (2^CHUNK_LOG, 8) chunks of a device vector in turn, through one host buffer"""
    buf = np.empty((1 << CHUNK_LOG, 8), dtype=np.uint32)
    for k in range(1 << (log_n - CHUNK_LOG)):
        cfg._check(msm_pkg.lib().msm_amd_copy_to_host(cfg.h, buf.ctypes.data_as(ctypes.c_void_p),
                                                      ctypes.c_void_p(d + (32 << CHUNK_LOG) * k), 32 << CHUNK_LOG))
        yield k, buf


def test_ntt_2_26(cfg, msm_pkg, dev):
    """2^26: passes of 9, 9 and 8 levels, the middle one (t = 9, low = 1); 2 GiB, in place.  The input is a random polynomial
    of 2^17 coefficients padded with zeros -- the low-degree extension a prover runs; it is dense after the first pass.  Then
    out[c + 512 j] = sum_i x_i (w^c)^i (w^512)^(i j) with w the 2^26-th root: the 2^17-point FORWARD transform of x with the
    shift w^c, at index j (that size and the shift are held to the model by tests/test_gpu_ntt_geometry.py; here the host
    twin computes it).  24 cosets c are compared with the strided slices of the big vector, among them 0, 1 and 511; then
    INVERSE in place gives x and zeros back, over the whole vector."""
    log_n, log_m, root, layout = shapes.MANY_WORKGROUPS[1][1], 17, m.ARK, m.MONT_LE
    n, small = 1 << log_n, 1 << log_m
    stride = n // small
    assert middle_pass(msm_pkg, log_n) == ([9, 9, 8], (9, 1)) and stride == 512
    x = m.np_random_records(26, small)
    cosets = sorted({0, 1, 2, 255, 256, 510, 511} | set(random.Random(26).sample(range(stride), 17)))
    assert len(cosets) >= 16
    w = m.omega(root, log_n)
    assert pow(w, stride, R) == m.omega(root, log_m)
    dom = cfg.ntt_domain(root, log_n)
    try:
        d = dev.alloc(32 * n)
        zeros = bytes(32 << CHUNK_LOG)
        for k in range(1 << (log_n - CHUNK_LOG)):
            cfg.to_device(d + (32 << CHUNK_LOG) * k, zeros)
        cfg.to_device(d, x.tobytes())
        cfg.ntt_device(dom, d, d, m.FORWARD, layout)
        got = {c: np.empty((small, 8), dtype=np.uint32) for c in cosets}
        per = (1 << CHUNK_LOG) // stride
        for k, chunk in read_chunks(msm_pkg, cfg, d, log_n):
            for c in cosets:
                got[c][k * per:(k + 1) * per] = chunk[c::stride]
        for c in cosets:
            exp = msm_pkg.host_ntt(x.tobytes(), root, log_m, m.FORWARD, layout, m.shift_record(pow(w, c, R), layout))
            same_records(got[c], exp, ("coset", c))
        cfg.ntt_device(dom, d, d, m.INVERSE, layout)
        for k, chunk in read_chunks(msm_pkg, cfg, d, log_n):
            if k == 0:
                same_records(chunk[:small], x, "round trip, the coefficients")
            rest = chunk[small:] if k == 0 else chunk
            assert not rest.any(), ("round trip, the padding", k, int(np.flatnonzero(rest.any(axis=1))[0]))
    finally:
        dom.free()


# ==== 5. what the audit found beside the four families: thresholds below 2^22 records that only a knob had crossed ================
def test_prefix_sum_three_levels_at_the_shipped_tile(cfg, msm_pkg, dev):
    """msm_amd_fr_prefix_sum_device at 2^18 + 1 records: the first size of three levels at tiles of 2^9, whose top tile holds two
    totals.  tests/test_gpu_lookup.py reaches three levels with MSM_AMD_FR_TILE_LOG only (the running products, which have
    kernels of their own, run 2^20 in tests/test_gpu_fr.py).  Dense reduced MONT_LE records and two edge words; the inclusive
    sums against the big-integer model, the exclusive ones are those moved on by one record; the twin agrees."""
    n, layout = (1 << 18) + 1, lr.MONT_LE
    assert [msm_pkg.test_fr_plan(k, 1, 9)["levels"] for k in (n - 1, n)] == [2, 3]
    data = lr.raw([R, (1 << 256) - 1]) + m.np_random_records(18, n - 2).tobytes()
    inclusive = lr.prefix_sum(data, layout, lr.INCLUSIVE)
    d_in, d_out = dev.put(data), dev.alloc(32 * n, FF)
    for mode, exp in ((lr.INCLUSIVE, inclusive), (lr.EXCLUSIVE, bytes(32) + inclusive[:-32])):
        assert msm_pkg.host_fr_prefix_sum(data, mode, layout) == exp
        cfg.fr_prefix_sum_device(d_in, n, d_out, mode, layout)
        same_records(cfg.to_host(d_out, 32 * n), exp, mode)
    assert cfg.to_host(d_in, 32 * n) == data
    cfg.fr_prefix_sum_device(d_in, n, d_in, lr.INCLUSIVE, layout)                  # in place
    same_records(cfg.to_host(d_in, 32 * n), inclusive, "in place")


@pytest.mark.parametrize("which", [2, 1], ids=["sixth-power", "one-factor-any"])
def test_sumcheck_terms_three_levels_at_the_shipped_chunk(cfg, msm_pkg, dev, which):
    """msm_amd_fr_sumcheck_round_terms at n = 2^20: 2048 waves of 2^8 pairs, so the partial sums fold twice (three launches).
    tests/test_gpu_sumcheck_terms.py stops at 2^16 with the default chunk and reaches three launches at
    MSM_AMD_FR_MLE_CHUNK_LOG = 6 only.  One and two tables of dense reduced MONT_LE records, both orders, against the host
    twin, which tests/test_sumcheck_terms_host.py pins to the model."""
    form, n, layout = t.FORMS[which], 1 << 20, lr.MONT_LE
    terms = form.lib_terms(msm_pkg, layout)
    assert [msm_pkg.test_fr_sumcheck_terms_plan(terms, k, form.n_vec)["launches"] for k in (n // 2, n)] == [2, 3]
    data = m.np_random_records(20 + which, n * form.n_vec).tobytes()
    d_in = dev.put(data)
    for order in t.ORDERS:
        twin = msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec, threads=16)
        assert len(twin) == 32 * (form.degree + 1)
        got, _ = cfg.fr_sumcheck_round_terms_device(d_in, n, terms, order, layout, form.n_vec)
        assert got == twin, (form, order)
    assert cfg.to_host(d_in, len(data)) == data
