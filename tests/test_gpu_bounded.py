"""GPU tests of the bounded-width calls (msm_amd_msm_bounded*, msm_amd_msm_g2_bounded*, msm_amd_scalar_width*): bounded
bytes == unbounded bytes == the big-integer model of bounded_ref.py over every window, size, width and scalar pattern,
through the device and host-buffer forms, prepared bases, table handles, batches and submit / wait, on G1 and G2; the plan
words and the digit stage against the model; violated bounds (status, message, untouched output, ctx still good); stale
workspaces; the width scan against its twin and the model."""
import ctypes
import re
import struct

import pytest

import bounded_ref as br
import g2_ref as g

pytestmark = pytest.mark.gpu

U, S = br.UNSIGNED, br.SIGNED
SIZES = [1, 31, 33, 257, (1 << 11) + 5, 1 << 13]   # the c = 3 policy edge, a second workgroup, the kDigitsSpan edge
WINDOWS = [3, 5, 13, 15, 16, 17, 0]               # forced; 0 = automatic.  Specialised and rolled kernels, u16 and u32 digits
PATTERN_WIDTHS = [1, 12, 13, 14, 16, 17, 18, 32, 63, 64, 65, 128, 253]


def on_device(cfg, data):
    d = cfg.alloc(max(1, len(data)))
    if data:
        cfg.to_device(d, data)
    return d


class Window:
    """msm_amd_set_window_size for the length of a test"""

    def __init__(self, cfg, c):
        self.cfg, self.c = cfg, c

    def __enter__(self):
        self.cfg.set_window_size(self.c)

    def __exit__(self, *a):
        self.cfg.set_window_size(0)


@pytest.fixture(scope="module")
def bases(cfg):
    """the progression bases of the largest size on the device, once: (host bytes, device pointer, discrete logs)"""
    pts, dl = br.g1_progression(max(SIZES))
    d = on_device(cfg, pts)
    yield pts, d, dl
    cfg.free(d)


def unbounded(cfg, ds, dp, n, layout, point_layout=0):
    return cfg.msm_batch_device([ds], [dp], [n], scalar_layout=layout, point_layout=point_layout)[0]


def check_call(cfg, msm_pkg, bases, n, ws, layout, bits, sign, c):
    """one vector through the bounded and the unbounded device call: bytes, model, plan words"""
    _, dp, dl = bases
    ds = on_device(cfg, br.encode(ws, layout))
    try:
        got = cfg.msm_bounded_device(ds, dp, n, bits, sign, scalar_layout=layout)
        plan = cfg.test_last_plan()
        assert got == unbounded(cfg, ds, dp, n, layout), (n, bits, sign, c)
    finally:
        cfg.free(ds)
    assert br.g1_decode(got) == br.g1_expected(ws, dl[:n]), (n, bits, sign, c)
    if c:
        assert plan["c"] == c
    assert plan["W_digits"] == bits // plan["c"] + 1 and plan["n_scalars"] == n, (plan, bits)
    return plan


# ---- every window x size x width, both signs --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", WINDOWS)
def test_bounded_equals_unbounded_equals_model(cfg, msm_pkg, bases, c, n):
    rng = br.rng_for("grid", c, n)
    with Window(cfg, c):
        for sign in (U, S):
            for i, bits in enumerate(br.widths_for(c or 15, sign)):
                name = br.PATTERNS[(i + n + sign) % len(br.PATTERNS)]
                layout = (i + sign) & 1
                check_call(cfg, msm_pkg, bases, n, br.pattern(name, n, bits, sign, rng, layout), layout, bits, sign, c)
        if not c:
            for bits in (8, 64):   # the automatic window is the published policy: a lone call here
                plan = check_call(cfg, msm_pkg, bases, n, br.pattern("random", n, bits, U, rng), br.CANON, bits, U, 0)
                assert plan["c"] == msm_pkg.auto_window_size_bounded(n, bits, lone=True)


# ---- every scalar pattern x layout x sign -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
@pytest.mark.parametrize("layout", [br.MONT, br.CANON])
@pytest.mark.parametrize("name", br.PATTERNS)
@pytest.mark.parametrize("c", [13, 17])
def test_scalar_patterns(cfg, msm_pkg, bases, c, name, layout, sign):
    n = (1 << 11) + 5
    rng = br.rng_for("patterns", c, name, layout, sign)
    with Window(cfg, c):
        for bits in PATTERN_WIDTHS:
            check_call(cfg, msm_pkg, bases, n, br.pattern(name, n, bits, sign, rng, layout), layout, bits, sign, c)


def test_signed_edges(cfg, msm_pkg, bases):
    """r - 1, r - (2^bits - 1), and at 253 bits the two residues around r / 2"""
    n = 257
    rng = br.rng_for("edges")
    for c in (5, 15, 16):
        with Window(cfg, c):
            for bits in (1, c, 2 * c, 64, 253):
                ws = [br.R - 1, br.R - ((1 << bits) - 1) if bits < 253 else br.HALF + 1, 1, 0, (1 << bits) - 1 if bits < 253 else br.HALF]
                ws += [br.signed_word(rng.randrange(1 << min(bits, 252)), rng.random() < 0.5) for _ in range(n - len(ws))]
                for layout in (br.MONT, br.CANON):
                    check_call(cfg, msm_pkg, bases, n, ws, layout, bits, S, c)
            ws = [br.HALF, br.HALF + 1, br.R - 1] + [rng.randrange(br.R) for _ in range(n - 3)]
            check_call(cfg, msm_pkg, bases, n, ws, br.MONT, 253, S, c)   # a signed call at 253 bits takes every residue


# ---- the other forms: host buffers, prepared bases, tables, batches, submit / wait ------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
def test_host_buffer_and_prepared_forms(cfg, msm_pkg, bases, sign):
    pts, dp, dl = bases
    n = (1 << 11) + 5
    rng = br.rng_for("forms", sign)
    d_prep = cfg.bases_prepare_device(dp, n)
    try:
        for bits in (1, 16, 33, 64, 128, 253):
            for layout in (br.MONT, br.CANON):
                ws = br.pattern("mixed", n, bits, sign, rng, layout)
                sc = br.encode(ws, layout)
                want = cfg.msm(sc, pts[:64 * n], n, scalar_layout=layout)
                assert br.g1_decode(want) == br.g1_expected(ws, dl[:n])
                assert cfg.msm_bounded(sc, pts[:64 * n], n, bits, sign, scalar_layout=layout) == want
                assert cfg.msm_bounded(sc, d_prep, n, bits, sign, scalar_layout=layout, point_layout=msm_pkg.POINT_PREPARED) == want
                ds = on_device(cfg, sc)
                try:
                    assert cfg.msm_bounded_device(ds, d_prep, n, bits, sign, scalar_layout=layout,
                                                  point_layout=msm_pkg.POINT_PREPARED) == want
                    assert cfg.test_last_plan()["W_digits"] == bits // cfg.test_last_plan()["c"] + 1
                finally:
                    cfg.free(ds)
    finally:
        cfg.free(d_prep)


@pytest.mark.parametrize("c", [5, 16, 0])
def test_tables_handle(cfg, msm_pkg, bases, c):
    """a bounded call runs on the first bits / c + 1 windows of the handle, at the handle's window"""
    pts, _, dl = bases
    n = 257
    rng = br.rng_for("tables", c)
    t = cfg.tables_build(pts[:64 * n], n, window_size=c)
    tc = cfg.tables_info(t)["window_size"]
    try:
        for sign in (U, S):
            for bits in (1, tc - 1, tc, tc + 1, 2 * tc, 64, 128, 253):
                ws = br.pattern("mixed", n, bits, sign, rng, br.CANON)
                ds = on_device(cfg, br.encode(ws, br.CANON))
                try:
                    got = cfg.msm_bounded_device(ds, t, n, bits, sign, scalar_layout=br.CANON, point_layout=msm_pkg.POINT_TABLES)
                    plan = cfg.test_last_plan()
                    assert got == unbounded(cfg, ds, t, n, br.CANON, msm_pkg.POINT_TABLES)
                    assert cfg.msm_bounded(br.encode(ws, br.CANON), t, n, bits, sign, scalar_layout=br.CANON,
                                           point_layout=msm_pkg.POINT_TABLES) == got
                finally:
                    cfg.free(ds)
                assert br.g1_decode(got) == br.g1_expected(ws, dl[:n])
                assert (plan["c"], plan["W"], plan["W_digits"], plan["n"]) == (tc, 1, bits // tc + 1, n * (bits // tc + 1))
    finally:
        cfg.tables_free(t)


@pytest.mark.parametrize("sign", [U, S])
def test_batch_of_three_and_submit_wait(cfg, msm_pkg, bases, sign):
    _, dp, dl = bases
    ns = [33, (1 << 11) + 5, 257]
    rng = br.rng_for("batch", sign)
    for bits in (1, 15, 32, 65, 128):
        wss = [br.pattern("mixed", n, bits, sign, rng, br.MONT) for n in ns]
        dss = [on_device(cfg, br.encode(ws, br.MONT)) for ws in wss]
        try:
            want = cfg.msm_batch_device(dss, [dp] * 3, ns)
            assert [br.g1_decode(w) for w in want] == [br.g1_expected(ws, dl[:n]) for ws, n in zip(wss, ns)]
            assert cfg.msm_batch_bounded_device(dss, [dp] * 3, ns, bits, sign) == want
            for j in range(3):
                plan = cfg.test_last_plan(j)
                assert plan["W_digits"] == bits // plan["c"] + 1 and plan["lone"] == 0
                assert plan["c"] == msm_pkg.auto_window_size_bounded(ns[j], bits, lone=False)
            first = cfg.submit_batch_bounded_device(dss, [dp] * 3, ns, bits, sign)
            second = cfg.submit_batch_bounded_device(dss[::-1], [dp] * 3, ns[::-1], bits, sign)
            assert cfg.wait_batch(first) == want and cfg.wait_batch(second) == want[::-1]
        finally:
            for d in dss:
                cfg.free(d)


# ---- G2: per call, prepared, tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
def test_g2_forms(cfg, msm_pkg, sign):
    n, a0, d = 257, 4242, 977
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(a0, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    dl = [a0 + i * d for i in range(n)]
    rng = br.rng_for("g2", sign)
    dp = on_device(cfg, pts)
    d_prep = cfg.g2_bases_prepare_device(dp, n)
    t = cfg.g2_tables_build(pts, n, window_size=9)
    try:
        for c in (5, 16, 0):
            with Window(cfg, c):
                for bits in (1, 8, 9, 10, 32, 65, 128, 253):
                    layout = bits & 1
                    ws = br.pattern("mixed", n, bits, sign, rng, layout)
                    sc = br.encode(ws, layout)
                    want = cfg.msm_g2(sc, pts, n, scalar_layout=layout)
                    assert g.decode_jacobian(want) == br.g2_expected(ws, dl)
                    assert cfg.msm_g2_bounded(sc, pts, n, bits, sign, scalar_layout=layout) == want
                    plan = cfg.test_g2_last_plan()
                    assert plan["W_digits"] == bits // plan["c"] + 1 and (not c or plan["c"] == c)
                    ds = on_device(cfg, sc)
                    try:
                        assert cfg.msm_g2_bounded_device(ds, dp, n, bits, sign, scalar_layout=layout) == want
                        assert cfg.msm_g2_bounded_device(ds, d_prep, n, bits, sign, scalar_layout=layout,
                                                         point_layout=msm_pkg.G2_POINT_PREPARED) == want
                        assert cfg.msm_g2_bounded_device(ds, t, n, bits, sign, scalar_layout=layout,
                                                         point_layout=msm_pkg.G2_POINT_TABLES) == want
                        plan = cfg.test_g2_last_plan()
                        assert (plan["c"], plan["W"], plan["W_digits"]) == (9, 1, bits // 9 + 1)
                    finally:
                        cfg.free(ds)
        ws = br.pattern("random", n, 32, sign, rng)
        ws[100] = br.signed_word(1 << 32, sign == S)
        out = ctypes.create_string_buffer(b"\x3c" * 192, 192)
        with pytest.raises(msm_pkg.MsmError) as e:
            cfg.msm_g2_bounded(br.encode(ws, br.CANON), pts, n, 32, sign, scalar_layout=br.CANON, out=out)
        assert e.value.status == msm_pkg.INPUT_ERROR and "1 record(s)" in str(e.value) and "index 100" in str(e.value)
        assert out.raw == b"\x3c" * 192
        ws[100] = 5
        assert g.decode_jacobian(cfg.msm_g2_bounded(br.encode(ws, br.CANON), pts, n, 32, sign, scalar_layout=br.CANON)) == \
            br.g2_expected(ws, dl)
    finally:
        cfg.g2_tables_free(t)
        cfg.free(d_prep)
        cfg.free(dp)


# ---- stage tap: the digits of a (c, bits) plan; the plan words at full width -------------------------------------------------
@pytest.mark.parametrize("n", [257, (1 << 11) + 5])
@pytest.mark.parametrize("c", [3, 5, 9, 10, 13, 15, 16, 17])   # 9 and 10: their compile-time (c, W) pairs at 8 and 127 bits
def test_stage_digits_equal_the_model(cfg, msm_pkg, bases, c, n):
    rng = br.rng_for("digits", c, n)
    with Window(cfg, c):
        for sign in (U, S):
            for bits in sorted({1, c - 1, c, c + 1, 2 * c, 33, 64, 127, 253}):
                ws = br.pattern("mixed", n, bits, sign, rng, br.CANON)
                check_call_digits(cfg, msm_pkg, bases, n, ws, bits, sign, c)


def check_call_digits(cfg, msm_pkg, bases, n, ws, bits, sign, c):
    _, dp, _ = bases
    ds = on_device(cfg, br.encode(ws, br.CANON))
    try:
        cfg.msm_bounded_device(ds, dp, n, bits, sign, scalar_layout=br.CANON)
        plan = cfg.test_last_plan()
        raw = cfg.test_stage_copy(msm_pkg.STAGE_DIGITS)
    finally:
        cfg.free(ds)
    W = bits // c + 1
    assert (plan["c"], plan["W_digits"], plan["wide_digits"]) == (c, W, int(c > 15))
    fmt = "<%d%s" % (W * n, "I" if c > 15 else "H")
    assert len(raw) == struct.calcsize(fmt)
    got = struct.unpack(fmt, raw)
    want = br.digit_matrix(ws, c, bits, sign)
    for w in range(W):
        assert list(got[w * n:(w + 1) * n]) == want[w], (c, bits, sign, w)


def plan_words(cfg, j=0):
    """the plan of instance j without the one word that is no plan: the round-robin workspace the instance ran in"""
    plan = cfg.test_last_plan(j)
    del plan["workspace"]
    return plan


@pytest.mark.parametrize("n", [33, (1 << 11) + 5])
def test_full_width_unsigned_is_the_unbounded_plan(cfg, msm_pkg, bases, n):
    _, dp, _ = bases
    ws = br.pattern("random", n, 254, U, br.rng_for("full", n))
    ds = on_device(cfg, br.encode(ws, br.MONT))
    try:
        for c in (0, 13, 16):
            with Window(cfg, c):
                a = cfg.msm_bounded_device(ds, dp, n, 254, U)
                plan_a = plan_words(cfg)
                b = unbounded(cfg, ds, dp, n, br.MONT)
                assert a == b and plan_a == plan_words(cfg)
                a3 = cfg.msm_batch_bounded_device([ds] * 3, [dp] * 3, [n] * 3, 254, U)
                plans_a = [plan_words(cfg, j) for j in range(3)]
                assert a3 == cfg.msm_batch_device([ds] * 3, [dp] * 3, [n] * 3) == [a] * 3
                assert plans_a == [plan_words(cfg, j) for j in range(3)]
    finally:
        cfg.free(ds)


# ---- violated bounds ------------------------------------------------------------------------------------------------------
def expect_violation(msm_pkg, call, count, indices, instance=None):
    with pytest.raises(msm_pkg.MsmError) as e:
        call()
    text = str(e.value)
    assert e.value.status == msm_pkg.INPUT_ERROR, text
    assert re.search(r"\b%d record\(s\)" % count, text), text
    m = re.search(r"index (\d+)", text)
    assert m and int(m.group(1)) in indices, text
    if instance is not None:
        assert "instance %d" % instance in text, text


@pytest.mark.parametrize("sign", [U, S])
@pytest.mark.parametrize("c", [5, 15, 17, 0])
def test_violations(cfg, msm_pkg, bases, c, sign):
    pts, dp, dl = bases
    n, bits = (1 << 11) + 5, 32
    rng = br.rng_for("violations", c, sign)
    pattern = b"\xa5" * 96
    with Window(cfg, c):
        for at in ([0], [n - 1], [1000], [3, 700, 701, n - 2]):   # the ends, a middle workgroup, several records
            ws = br.pattern("random", n, bits, sign, rng)
            for i in at:
                ws[i] = br.signed_word(1 << bits, sign == S)   # magnitude exactly 2^bits
            sc = br.encode(ws, br.CANON)
            ds = on_device(cfg, sc)
            try:
                out = ctypes.create_string_buffer(pattern, 96)
                expect_violation(msm_pkg, lambda: cfg.msm_bounded_device(ds, dp, n, bits, sign, scalar_layout=br.CANON, out=out),
                                 len(at), at)
                assert out.raw == pattern
                expect_violation(msm_pkg, lambda: cfg.msm_bounded(sc, pts[:64 * n], n, bits, sign, scalar_layout=br.CANON, out=out),
                                 len(at), at)
                assert out.raw == pattern
                # the same records are inside a bound one bit wider, and the ctx goes on
                got = cfg.msm_bounded_device(ds, dp, n, bits + 1, sign, scalar_layout=br.CANON)
                assert got == unbounded(cfg, ds, dp, n, br.CANON) and br.g1_decode(got) == br.g1_expected(ws, dl[:n])
            finally:
                cfg.free(ds)


def test_violation_in_instance_1_of_a_batch(cfg, msm_pkg, bases):
    _, dp, dl = bases
    ns, bits = [257, 33, (1 << 11) + 5], 16
    rng = br.rng_for("batch violation")
    wss = [br.pattern("random", n, bits, U, rng) for n in ns]
    wss[1][20] = 1 << bits
    dss = [on_device(cfg, br.encode(ws, br.CANON)) for ws in wss]
    try:
        pattern = b"\x77" * (96 * 3)
        out = ctypes.create_string_buffer(pattern, len(pattern))
        expect_violation(msm_pkg, lambda: cfg.msm_batch_bounded_device(dss, [dp] * 3, ns, bits, U, scalar_layout=br.CANON, out=out),
                         1, [20], instance=1)
        assert out.raw == pattern
        h = cfg.submit_batch_bounded_device(dss, [dp] * 3, ns, bits, U, scalar_layout=br.CANON, out=out)
        expect_violation(msm_pkg, lambda: cfg.wait_batch(h), 1, [20], instance=1)
        assert out.raw == pattern
        got = cfg.msm_batch_bounded_device(dss, [dp] * 3, ns, bits + 1, U, scalar_layout=br.CANON)
        assert [br.g1_decode(x) for x in got] == [br.g1_expected(ws, dl[:n]) for ws, n in zip(wss, ns)]
    finally:
        for d in dss:
            cfg.free(d)


def test_device_argument_errors(cfg, msm_pkg, bases):
    pts, dp, _ = bases
    sc = br.encode([1, 2, 3], br.CANON)
    ds = on_device(cfg, sc)
    try:
        for bits, sign in ((0, U), (255, U), (254, S), (8, 2), (8, -1)):
            for call in (lambda: cfg.msm_bounded_device(ds, dp, 3, bits, sign, scalar_layout=br.CANON),
                         lambda: cfg.msm_bounded(sc, pts[:192], 3, bits, sign, scalar_layout=br.CANON),
                         lambda: cfg.msm_batch_bounded_device([ds], [dp], [3], bits, sign, scalar_layout=br.CANON),
                         lambda: cfg.submit_batch_bounded_device([ds], [dp], [3], bits, sign, scalar_layout=br.CANON),
                         lambda: cfg.msm_g2_bounded_device(ds, dp, 3, bits, sign, scalar_layout=br.CANON),
                         lambda: cfg.msm_g2_bounded(sc, bytes(384), 3, bits, sign, scalar_layout=br.CANON)):
                with pytest.raises(msm_pkg.MsmError) as e:
                    call()
                assert e.value.status == msm_pkg.INPUT_ERROR and ("bits must be" in str(e.value) or "sign must be" in str(e.value))
        for call in (lambda: cfg.scalar_width_device(ds, 3, 2, br.CANON), lambda: cfg.scalar_width(sc, 3, U, 2),
                     lambda: cfg.scalar_width_device(None, 3, U, br.CANON), lambda: cfg.scalar_width(sc, 1 << 32, U, br.CANON)):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.INPUT_ERROR and "msm_amd_scalar_width" in str(e.value)
        assert cfg.msm_bounded_device(ds, dp, 3, 2, U, scalar_layout=br.CANON) == unbounded(cfg, ds, dp, 3, br.CANON)
    finally:
        cfg.free(ds)


# ---- stale state: more windows first, then fewer -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", [5, 15, 17])
def test_narrow_call_after_a_wide_one_on_filled_workspaces(cfg, msm_pkg, bases, c):
    _, dp, dl = bases
    n = (1 << 11) + 5
    rng = br.rng_for("stale", c)
    wide = br.pattern("random", n, 254, U, rng)
    d_wide = on_device(cfg, br.encode(wide, br.CANON))
    try:
        with Window(cfg, c):
            for fill in (0x00, 0xFF, 0xA5):
                for bits in (1, c, 40):
                    for _ in range(4):   # every workspace of the ctx sees the wide plan, then the narrow one
                        assert br.g1_decode(unbounded(cfg, d_wide, dp, n, br.CANON)) == br.g1_expected(wide, dl[:n])
                    cfg.test_fill_workspaces(fill)
                    ws = br.pattern("mixed", n, bits, S, rng)
                    ds = on_device(cfg, br.encode(ws, br.CANON))
                    try:
                        for _ in range(4):
                            assert br.g1_decode(cfg.msm_bounded_device(ds, dp, n, bits, S, scalar_layout=br.CANON)) == \
                                br.g1_expected(ws, dl[:n]), (c, fill, bits)
                    finally:
                        cfg.free(ds)
    finally:
        cfg.free(d_wide)


# ---- width scan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
@pytest.mark.parametrize("layout", [br.MONT, br.CANON])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, (1 << 14) + 3])
def test_width_scan(cfg, msm_pkg, n, layout, sign):
    rng = br.rng_for("scan", n, layout, sign)
    cases = [(name, bits) for name in br.PATTERNS for bits in ((1, 33, 253) if n > 1000 else (1, 8, 32, 33, 64, 128, 253))]
    for name, bits in cases if n else [("zero", 1)]:
        ws = br.pattern(name, n, bits, sign, rng, layout) if n else []
        sc = br.encode(ws, layout)
        want = br.width(ws, sign)
        ds = on_device(cfg, sc)
        try:
            assert cfg.scalar_width_device(ds, n, sign, layout) == want, (name, bits)
        finally:
            cfg.free(ds)
        assert cfg.scalar_width(sc, n, sign, layout) == want, (name, bits)
        assert msm_pkg.host_scalar_width(sc, n, sign, layout, threads=3) == want, (name, bits)


def test_width_scan_ties_pick_the_lowest_index(cfg, msm_pkg):
    n = (1 << 14) + 3
    for at in ([5, 64, 1023, 1024, n - 1], [n - 1], [1024 * 9 + 1, 1024 * 9 + 65], [0, n - 1]):
        ws = [7] * n
        for i in at:
            ws[i] = 1 << 77
        ws[at[-1]] = (1 << 78) - 1   # as wide as the others
        sc = br.encode(ws, br.CANON)
        assert cfg.scalar_width(sc, n, U, br.CANON) == (78, {"zeros": 0, "negatives": 0, "widest": at[0]})
        ws[at[0]] = br.R - (1 << 77)
        want = br.width(ws, S)
        assert want[1]["widest"] == at[0] and want[1]["negatives"] == 1
        assert cfg.scalar_width(br.encode(ws, br.CANON), n, S, br.CANON) == want == \
            msm_pkg.host_scalar_width(br.encode(ws, br.CANON), n, S, br.CANON)


def test_scan_then_commit_at_that_width(cfg, msm_pkg, bases):
    """the INTEGRATION.md recipe: the width of a witness, then the MSM at that width"""
    _, dp, dl = bases
    n = 1 << 13
    rng = br.rng_for("recipe")
    ws = [br.signed_word(rng.randrange(1 << rng.choice((1, 8, 32, 64))), rng.random() < 0.1) for _ in range(n)]
    ds = on_device(cfg, br.encode(ws, br.MONT))
    try:
        bits, stats = cfg.scalar_width_device(ds, n, S)
        assert (bits, stats) == br.width(ws, S) and bits <= 64
        got = cfg.msm_bounded_device(ds, dp, n, bits, S)
        assert got == unbounded(cfg, ds, dp, n, br.MONT) and br.g1_decode(got) == br.g1_expected(ws, dl)
        if bits > 1:
            with pytest.raises(msm_pkg.MsmError):
                cfg.msm_bounded_device(ds, dp, n, bits - 1, S)
    finally:
        cfg.free(ds)
