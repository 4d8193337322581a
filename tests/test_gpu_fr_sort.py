"""The sort of Fr records by canonical value on the GPU (msm_amd_fr_sort) against the host twin and the model of
tests/sort_ref.py (tests/test_fr_sort_host.py pins the twin to the model on the CPU).  Every comparison is of bytes: ctx call =
twin = model for both `mem` forms, into buffers that start as 0xFF bytes, and the inputs of an out-of-place call are as they
were afterwards.  The sizes lie round the wave (64), the quarter of a tile one wave owns (1024) and the tile (4096) of a
pass; the columns of the digit-skipping tests are built so that the keys differ in chosen bytes only, and the plan of that
mask is compared with the header's definition."""
import ctypes
import random

import pytest

import lookup_ref as lr
import sort_ref as sr
from guard import Arena, HostArena, In, Out, guarded

pytestmark = pytest.mark.gpu

R = sr.R
FF = b"\xFF"
MEMS = (sr.MEM_HOST, sr.MEM_DEVICE)


def prefilled(nbytes):
    return ctypes.create_string_buffer(FF * nbytes, nbytes)


def device_sort(cfg, data, layout, n_vec, want_out=True, want_perm=True, in_place=False):
    """MEM_DEVICE on fresh device buffers that start as 0xFF: (out bytes or None, perm list or None, the input afterwards)"""
    total = len(data) // 32
    d_in, d_out, d_perm = cfg.alloc(len(data)), cfg.alloc(len(data)), cfg.alloc(4 * total)
    try:
        cfg.to_device(d_in, data)
        cfg.to_device(d_out, FF * len(data))
        cfg.to_device(d_perm, FF * 4 * total)
        o = (d_in if in_place else d_out) if want_out else None
        cfg.fr_sort(d_in, layout, n_vec, sr.MEM_DEVICE, n=total // n_vec, out=o, perm_out=d_perm if want_perm else None)
        out, perm, src = cfg.to_host(d_out, len(data)), cfg.to_host(d_perm, 4 * total), cfg.to_host(d_in, len(data))
    finally:
        for p in (d_in, d_out, d_perm):
            cfg.free(p)
    words = [int.from_bytes(perm[i:i + 4], "little") for i in range(0, len(perm), 4)]
    if in_place:
        return (src if want_out else None), (words if want_perm else None), None
    assert want_out or out == FF * len(data)
    assert want_perm or perm == FF * 4 * total
    return (out if want_out else None), (words if want_perm else None), src


def check(cfg, msm_pkg, data, layout, n_vec=1, mask=None, tag=None):
    """ctx call = twin = model in both mem forms; mask: the digit mask the column was built for"""
    exp_out, exp_perm = sr.sort(data, layout, n_vec)
    total = len(data) // 32
    assert msm_pkg.host_fr_sort(data, layout, n_vec) == (exp_out, exp_perm), tag
    src, out = ctypes.create_string_buffer(data, len(data)), prefilled(len(data))
    perm = (ctypes.c_uint32 * total)(*([0xFFFFFFFF] * total))
    assert cfg.fr_sort(src, layout, n_vec, sr.MEM_HOST, n=total // n_vec, out=out, perm_out=perm)[:2] == (None, None), tag
    assert sr.first_difference(out.raw, exp_out) is None, (tag, "host out")
    assert list(perm) == exp_perm, (tag, "host perm")
    assert src.raw == data, tag
    d_out, d_perm, d_src = device_sort(cfg, data, layout, n_vec)
    assert sr.first_difference(d_out, exp_out) is None, (tag, "device out")
    assert d_perm == exp_perm, (tag, "device perm")
    assert d_src == data, tag
    if mask is not None:
        assert sr.digit_mask(data, layout) == mask, tag
        got, exp = msm_pkg.test_fr_sort_plan(total // n_vec, n_vec, mask), sr.plan(total // n_vec, n_vec, mask)
        assert {k: got[k] for k in exp} == exp, tag
    return exp_out, exp_perm


# ---- 1. sizes across the wave, the quarter tile of a wave and the tile ----------------------------------------------------------
@pytest.mark.parametrize("n", sr.SIZES)
def test_sizes(cfg, msm_pkg, n):
    for layout in sr.LAYOUTS:
        check(cfg, msm_pkg, sr.random_column(n + layout, n, layout), layout, tag=(n, layout))


# ---- 2. few distinct values: long runs, perm ascends inside every one -----------------------------------------------------------
@pytest.mark.parametrize("layout", sr.LAYOUTS)
def test_few_distinct_values(cfg, msm_pkg, layout):
    data = sr.few_values(5, 5000, layout, 5)
    out, perm = check(cfg, msm_pkg, data, layout)
    sr.runs_ascend(data, perm, layout)
    assert len(set(sr.words(out))) == 5


# ---- 3. records equal mod r under different words ---------------------------------------------------------------------------------
def test_records_equal_mod_r(cfg, msm_pkg):
    xs = [5, 0, (1 << 253) + 7, 1]
    ws = [x + k * R for x in xs for k in (4, 1, 0) if x + k * R < (1 << 256)]
    random.Random(3).shuffle(ws)
    out, perm = check(cfg, msm_pkg, sr.raw(ws), sr.CANON_LE, tag="x + k r")
    assert sr.words(out) == sorted(w % R for w in ws)
    for layout in sr.LAYOUTS:
        out, perm = check(cfg, msm_pkg, lr.edge_records(layout) * 3, layout, tag="edge")
        assert all(w < R for w in sr.words(out))


# ---- 4. the order is that of the value, not that of the Montgomery words ---------------------------------------------------------
def test_order_is_by_value_not_by_montgomery_words(cfg, msm_pkg):
    data = sr.random_column(11, 300, sr.MONT_LE)
    out, perm = check(cfg, msm_pkg, data, sr.MONT_LE)
    assert perm != sorted(range(300), key=lambda i: (sr.words(data)[i], i))      # the two orders differ on this column
    assert sr.decode(out, sr.MONT_LE) == sorted(sr.decode(data, sr.MONT_LE))


# ---- 5. digit skipping: columns whose keys differ in chosen bytes only -----------------------------------------------------------
def skipping_columns(n):
    rng = random.Random(n)
    yield "below 2^16", [rng.randrange(1 << 16) for _ in range(n)], 0x3
    yield "top byte", [(rng.randrange(0x30) << 248) + 5 for _ in range(n)], 0x80000000
    yield "bytes 0 and 17", [rng.randrange(256) + (rng.randrange(256) << 136) + (3 << 64) for _ in range(n)], 0x00020001
    yield "all equal", [R - 2] * n, 0
    yield "ascending", [7 * i for i in range(n)], 0x3
    yield "descending", [7 * (n - i) for i in range(n)], 0x3


@pytest.mark.parametrize("layout", sr.LAYOUTS)
def test_digit_skipping(cfg, msm_pkg, layout):
    n = 4500
    for name, vals, mask in skipping_columns(n):
        out, perm = check(cfg, msm_pkg, sr.encode(vals, layout), layout, mask=mask, tag=name)
        if name in ("all equal", "ascending"):
            assert perm == list(range(n)), name
        if name == "descending":
            assert perm == list(range(n - 1, -1, -1)), name


# ---- 6. several columns: a boundary inside a wave and inside a tile; indices are column-relative ---------------------------------
@pytest.mark.parametrize("n", [65, 4097])
def test_columns(cfg, msm_pkg, n):
    for layout in sr.LAYOUTS:
        cols = sr.random_column(1, n, layout) + sr.encode([7] * n, layout) + sr.random_column(2, n, layout)
        out, perm = check(cfg, msm_pkg, cols, layout, n_vec=3, tag=n)
        assert perm[n:2 * n] == list(range(n)) and max(perm) == n - 1


# ---- 7. forms: in place, one output only, nothing to do --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sr.LAYOUTS)
def test_forms(cfg, msm_pkg, layout):
    n_vec, n = 2, 1500
    data = sr.random_column(21, n, layout) + sr.few_values(22, n, layout, 3)
    exp_out, exp_perm = sr.sort(data, layout, n_vec)
    buf = ctypes.create_string_buffer(data, len(data))
    assert cfg.fr_sort(buf, layout, n_vec, n=n, out=buf)[:2] == (None, exp_perm) and buf.raw == exp_out      # out == in
    assert cfg.fr_sort(data, layout, n_vec, want_perm=False)[:2] == (exp_out, None)
    assert cfg.fr_sort(data, layout, n_vec, want_out=False)[:2] == (None, exp_perm)
    assert device_sort(cfg, data, layout, n_vec, in_place=True)[:2] == (exp_out, exp_perm)
    assert device_sort(cfg, data, layout, n_vec, want_perm=False) == (exp_out, None, data)
    assert device_sort(cfg, data, layout, n_vec, want_out=False) == (None, exp_perm, data)
    out = prefilled(64)
    for n, n_vec in ((5, 0), (0, 5)):                      # nothing to do: no pointer is looked at but for being there
        assert cfg.fr_sort(None, layout, n_vec, sr.MEM_HOST, n=n, out=out, want_perm=False)[:2] == (None, None)
        assert cfg.fr_sort(None, layout, n_vec, sr.MEM_DEVICE, n=n, perm_out=16)[:2] == (None, None)
    assert out.raw == FF * 64


# ---- 8. every argument error, before any launch ----------------------------------------------------------------------------------
def test_argument_errors(cfg, msm_pkg):
    L = msm_pkg.lib()
    layout = sr.MONT_LE
    n = 8
    data = sr.random_column(1, n, layout)
    d = cfg.alloc(32 * 64)
    h = ctypes.create_string_buffer(32 * 64)
    P = ctypes.c_void_p
    try:
        cfg.to_device(d, data + FF * (32 * 64 - len(data)))
        ctypes.memmove(h, data, len(data))
        for mem, at in ((sr.MEM_DEVICE, d), (sr.MEM_HOST, ctypes.addressof(h))):
            good = dict(mem=mem, layout=layout, data=P(at), n=n, n_vec=1, out=P(at + 32 * 16), perm=P(at + 32 * 32))

            def call(**kw):
                x = dict(good, **kw)
                return L.msm_amd_fr_sort(cfg.h, x["mem"], x["layout"], x["data"], x["n"], x["n_vec"], x["out"], x["perm"], None)
            errors = dict(unknown_mem=dict(mem=2), negative_mem=dict(mem=-1), unknown_layout=dict(layout=msm_pkg.SCALAR_CANON_BE32),
                          null_in=dict(data=None), no_output=dict(out=None, perm=None), n_2_32=dict(n=1 << 32),
                          product_2_32=dict(n=1 << 16, n_vec=1 << 16),
                          out_over_in=dict(out=P(at + 32 * 3)), out_under_in=dict(data=P(at + 32), out=P(at)),
                          perm_in_in=dict(perm=P(at + 32 * 3)), perm_in_out=dict(perm=P(at + 32 * 16 + 32 * n - 4)),
                          perm_over_out=dict(out=P(at + 32 * 32 + 16)))
            if mem == sr.MEM_DEVICE:
                errors.update(misaligned_in=dict(data=P(at + 8)), misaligned_out=dict(out=P(at + 32 * 16 + 4)),
                              misaligned_perm=dict(perm=P(at + 32 * 32 + 2)))
            for name, kw in errors.items():
                assert call(**kw) == msm_pkg.INPUT_ERROR, (mem, name)
            assert call(n=0, out=None, perm=None) == msm_pkg.INPUT_ERROR and call(n=0, layout=99) == msm_pkg.INPUT_ERROR
            assert call() == msm_pkg.OK and call(out=good["data"]) == msm_pkg.OK, mem                # and in place
        assert L.msm_amd_fr_sort(None, 0, layout, h, n, 1, h, None, None) == msm_pkg.INPUT_ERROR
        exp_out, exp_perm = sr.sort(data, layout)
        assert cfg.to_host(d, 32 * n) == exp_out == h.raw[:32 * n]                                    # the refused calls wrote nothing
        assert cfg.to_host(d + 32 * n, 32 * 8) == FF * 32 * 8 and h.raw[32 * n:32 * 16] == bytes(32 * (16 - n))
    finally:
        cfg.free(d)


# ---- 9. guard bands round out and perm_out, both mem forms ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4097])
@pytest.mark.parametrize("mem", MEMS)
def test_guard_bands(cfg, msm_pkg, mem, n):
    layout, n_vec = sr.CANON_LE, 2
    data = sr.random_column(n, n, layout) + sr.random_column(n + 1, n, layout, below=1 << 20)
    exp_out, exp_perm = sr.sort(data, layout, n_vec)
    fn = msm_pkg.lib().msm_amd_fr_sort
    with (Arena(cfg) if mem == sr.MEM_DEVICE else HostArena()) as arena:
        out, perm = guarded(arena, fn, cfg.h, mem, layout, In(data), n, n_vec, Out(len(data)), Out(4 * n * n_vec), None)
    assert out == exp_out and [int.from_bytes(perm[i:i + 4], "little") for i in range(0, len(perm), 4)] == exp_perm
    with (Arena(cfg) if mem == sr.MEM_DEVICE else HostArena()) as arena:
        both = Out(data=data)
        out, = guarded(arena, fn, cfg.h, mem, layout, both, n, n_vec, both, None, None)          # in place, no perm_out
    assert out == exp_out
