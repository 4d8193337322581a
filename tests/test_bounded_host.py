"""CPU tests of the bounded-width calls: the host twins (msm_amd_host_msm_bounded, msm_amd_host_msm_g2_bounded,
msm_amd_host_scalar_width) against the big-integer model of bounded_ref.py and against the unbounded twins, violated
bounds, every argument error, the exports and the window policy at full width."""
import ctypes

import pytest

import bounded_ref as br
import g2_ref as g

U, S = br.UNSIGNED, br.SIGNED


def raises_input_error(msm_pkg, fn, *a, **kw):
    with pytest.raises(msm_pkg.MsmError) as e:
        fn(*a, **kw)
    assert e.value.status == msm_pkg.INPUT_ERROR


# ---- the model itself --------------------------------------------------------------------------------------------------
def test_model_fold_and_digits():
    assert br.magnitude(br.R - 1, S) == (1, True) and br.magnitude(br.R - 1, U) == (br.R - 1, False)
    assert br.magnitude(br.HALF, S) == (br.HALF, False) and br.magnitude(br.HALF + 1, S) == (br.HALF, True)
    assert br.HALF.bit_length() == 253 and (br.R - 1).bit_length() == 254
    rng = br.rng_for("model")
    for c in (3, 5, 13, 15, 16, 17):
        for bits in br.widths_for(c, S):
            for sign in (U, S):
                for w in br.pattern("mixed", 12, bits, sign, rng) + br.pattern("max", 2, bits, sign, rng):
                    d = br.digits(w, c, bits, sign)
                    assert len(d) == bits // c + 1 and all(abs(v) <= 1 << (c - 1) for v in d)
                    assert sum(v << (c * i) for i, v in enumerate(d)) % br.R == (w % br.R if sign == U or w % br.R <= br.HALF
                                                                               else w % br.R - br.R) % br.R


# ---- G1 twin == model == unbounded twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
@pytest.mark.parametrize("layout", [br.MONT, br.CANON])
@pytest.mark.parametrize("n", [1, 31, 33, 257])
def test_host_msm_bounded_equals_model_and_unbounded(msm_pkg, n, layout, sign):
    pts, dl = br.g1_progression(257)
    pts, dl = pts[:64 * n], dl[:n]
    rng = br.rng_for("host", n, layout, sign)
    for bits in (1, 2, 8, 13, 31, 32, 33, 64, 65, 128, 253) + ((254,) if sign == U else ()):
        for name in ("mixed", "max", "zero"):
            ws = br.pattern(name, n, bits, sign, rng, layout)
            sc = br.encode(ws, layout)
            got = msm_pkg.host_msm_bounded(sc, pts, n, bits, sign, threads=3, scalar_layout=layout)
            assert got == msm_pkg.host_msm(sc, pts, n, threads=3, scalar_layout=layout), (bits, name)
            assert br.g1_decode(got) == br.g1_expected(ws, dl), (bits, name)


def test_host_msm_bounded_threads_agree(msm_pkg):
    n = 257
    pts, dl = br.g1_progression(257)
    ws = br.pattern("random", n, 64, S, br.rng_for("threads"))
    sc = br.encode(ws, br.CANON)
    outs = {msm_pkg.host_msm_bounded(sc, pts, n, 64, S, threads=t, scalar_layout=br.CANON) for t in (1, 3, 16)}
    assert len(outs) == 1 and br.g1_decode(outs.pop()) == br.g1_expected(ws, dl)


@pytest.mark.parametrize("sign", [U, S])
def test_host_msm_bounded_violation_leaves_output(msm_pkg, sign):
    n, bits = 65, 32
    pts, _ = br.g1_progression(257)
    rng = br.rng_for("viol", sign)
    for at in (0, n - 1, 40):
        ws = br.pattern("random", n, bits, sign, rng)
        ws[at] = br.signed_word(1 << bits, sign == S)   # magnitude exactly 2^bits
        out = ctypes.create_string_buffer(b"\xa5" * 96, 96)
        raises_input_error(msm_pkg, msm_pkg.host_msm_bounded, br.encode(ws, br.CANON), pts[:64 * n], n, bits, sign, 3, br.CANON,
                           out=out)
        assert out.raw == b"\xa5" * 96
        ws[at] = br.signed_word((1 << bits) - 1, sign == S)
        msm_pkg.host_msm_bounded(br.encode(ws, br.CANON), pts[:64 * n], n, bits, sign, 3, br.CANON)


def test_signed_253_takes_every_residue(msm_pkg):
    n = 33
    pts, dl = br.g1_progression(257)
    rng = br.rng_for("all")
    ws = [br.R - 1, br.HALF, br.HALF + 1, 0, 1] + [rng.randrange(br.R) for _ in range(n - 5)]
    sc = br.encode(ws, br.MONT)
    got = msm_pkg.host_msm_bounded(sc, pts[:64 * n], n, 253, S, threads=2)
    assert got == msm_pkg.host_msm(sc, pts[:64 * n], n, threads=2) and br.g1_decode(got) == br.g1_expected(ws, dl)


# ---- G2 twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
def test_host_msm_g2_bounded_equals_model_and_unbounded(msm_pkg, sign):
    n, a0, d = 33, 77, 1001
    pts = msm_pkg.g2_progression(g.encode_h2c(g.scalar_mul(a0, g.GEN2)), g.encode_h2c(g.scalar_mul(d, g.GEN2)), n)
    dl = [a0 + i * d for i in range(n)]
    rng = br.rng_for("g2host", sign)
    for layout in (br.MONT, br.CANON):
        for bits in (1, 8, 32, 65, 128, 253):
            ws = br.pattern("mixed", n, bits, sign, rng, layout)
            sc = br.encode(ws, layout)
            got = msm_pkg.host_msm_g2_bounded(sc, pts, n, bits, sign, threads=2, scalar_layout=layout)
            assert got == msm_pkg.host_msm_g2(sc, pts, n, threads=2, scalar_layout=layout)
            assert g.decode_jacobian(got) == br.g2_expected(ws, dl)
    ws[7] = br.signed_word(1 << 253, False) if sign == U else ws[7]
    if sign == U:
        out = ctypes.create_string_buffer(b"\x5a" * 192, 192)
        raises_input_error(msm_pkg, msm_pkg.host_msm_g2_bounded, br.encode(ws, br.CANON), pts, n, 253, U, 2, br.CANON, out=out)
        assert out.raw == b"\x5a" * 192


# ---- width twin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [U, S])
@pytest.mark.parametrize("layout", [br.MONT, br.CANON])
def test_host_scalar_width(msm_pkg, layout, sign):
    rng = br.rng_for("width", layout, sign)
    assert msm_pkg.host_scalar_width(b"", 0, sign, layout) == (0, {"zeros": 0, "negatives": 0, "widest": 0})
    for n in (1, 63, 64, 65, 1000):
        for bits in (1, 8, 32, 33, 64, 128, 253):
            for name in br.PATTERNS:
                ws = br.pattern(name, n, bits, sign, rng, layout)
                want = br.width(ws, sign)
                for threads in (1, 3, 16):
                    assert msm_pkg.host_scalar_width(br.encode(ws, layout), n, sign, layout, threads) == want, (n, bits, name)


def test_host_scalar_width_ties_pick_lowest_index(msm_pkg):
    ws = [3, 0, 1 << 40, 5, (1 << 41) - 1, 1 << 40, 1 << 39] + [7] * 200 + [1 << 40]   # 41 bits at 2, 4, 5 and the end
    for threads in (1, 3, 16):
        assert msm_pkg.host_scalar_width(br.encode(ws, br.CANON), len(ws), U, br.CANON, threads) == \
            (41, {"zeros": 1, "negatives": 0, "widest": 2})
    ws[1] = br.R - (1 << 40)   # signed: as wide as the others, and in front of them
    assert msm_pkg.host_scalar_width(br.encode(ws, br.MONT), len(ws), S, br.MONT, 3) == \
        (41, {"zeros": 0, "negatives": 1, "widest": 1})
    assert msm_pkg.host_scalar_width(br.encode(ws, br.MONT), len(ws), U, br.MONT, 3) == \
        (254, {"zeros": 0, "negatives": 0, "widest": 1})


# ---- argument errors, by name --------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    pts, _ = br.g1_progression(257)
    sc = br.encode([1, 2, 3], br.CANON)
    bad = [
        dict(bits=0), dict(bits=255), dict(bits=254, sign=S), dict(bits=8, sign=2), dict(bits=8, sign=-1),
        dict(bits=8, scalar_layout=2), dict(bits=8, scalar_layout=7), dict(bits=8, point_layout=msm_pkg.POINT_ARK_AFFINE),
    ]
    for kw in bad:
        kw = dict(dict(sign=U, scalar_layout=br.CANON), **kw)
        raises_input_error(msm_pkg, msm_pkg.host_msm_bounded, sc, pts, 3, threads=1, **kw)
    raises_input_error(msm_pkg, msm_pkg.host_msm_bounded, sc, pts, 0, 8)
    raises_input_error(msm_pkg, msm_pkg.host_msm_bounded, None, pts, 3, 8)
    g2pts = bytes(128 * 3)
    for kw in (dict(bits=0), dict(bits=255), dict(bits=254, sign=S), dict(bits=8, sign=2), dict(bits=8, point_layout=9)):
        raises_input_error(msm_pkg, msm_pkg.host_msm_g2_bounded, sc, g2pts, 3, threads=1, **dict(dict(sign=U), **kw))
    raises_input_error(msm_pkg, msm_pkg.host_scalar_width, sc, 3, 2, br.CANON)
    raises_input_error(msm_pkg, msm_pkg.host_scalar_width, sc, 3, U, 2)       # CANON_BE32 is not taken
    raises_input_error(msm_pkg, msm_pkg.host_scalar_width, None, 3, U, br.CANON)
    L = msm_pkg.lib()
    assert L.msm_amd_host_scalar_width(br.CANON, sc, 3, U, 1, None, None) == msm_pkg.INPUT_ERROR   # bits is required
    bits = ctypes.c_uint32(99)
    assert L.msm_amd_host_scalar_width(br.CANON, sc, 3, U, 1, ctypes.byref(bits), None) == msm_pkg.OK and bits.value == 2
    # without a ctx the device entry points refuse before anything else
    for fn in ("msm_amd_msm_bounded", "msm_amd_msm_bounded_device", "msm_amd_msm_g2_bounded", "msm_amd_msm_g2_bounded_device"):
        assert getattr(L, fn)(None, br.CANON, 0, sc, pts, 3, 8, U, ctypes.create_string_buffer(192)) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_scalar_width(None, br.CANON, sc, 3, U, ctypes.byref(bits), None) == msm_pkg.INPUT_ERROR


def test_abi_exports(msm_pkg):
    names = ["msm_amd_scalar_width", "msm_amd_scalar_width_device", "msm_amd_host_scalar_width", "msm_amd_msm_bounded",
             "msm_amd_msm_bounded_device", "msm_amd_msm_batch_bounded_device", "msm_amd_submit_batch_bounded_device",
             "msm_amd_msm_g2_bounded", "msm_amd_msm_g2_bounded_device", "msm_amd_host_msm_bounded",
             "msm_amd_host_msm_g2_bounded", "msm_amd_auto_window_size_bounded"]
    L = msm_pkg.lib()
    for name in names:
        assert name in msm_pkg.EXPORTS and hasattr(L, name), name
    assert (msm_pkg.WIDTH_UNSIGNED, msm_pkg.WIDTH_SIGNED) == (0, 1)


def test_window_policy_at_full_width_is_the_existing_policy(msm_pkg):
    L = msm_pkg.lib()
    for log_n in range(0, 27):
        for n in {max(1, (1 << log_n) - 1), 1 << log_n, (1 << log_n) + 1}:
            assert msm_pkg.auto_window_size_bounded(n, 254, lone=False) == L.msm_amd_auto_window_size(n)
            assert msm_pkg.auto_window_size_bounded(n, 254, lone=True) == L.msm_amd_auto_window_size_lone(n)
    # the rule profiles/bounded_sweep.txt supports: one full window up to 16 bits, the fewest windows with a wide top digit
    # above, c <= 13 for small instances, the unbounded window below the swept sizes
    for n, bits, lone, c in ((1 << 20, 8, False, 9), (1 << 22, 8, True, 9), (1 << 20, 16, False, 17), (1 << 20, 32, True, 17),
                             (1 << 22, 64, False, 17), (1 << 20, 128, False, 10), (1 << 22, 128, True, 10), (1 << 18, 64, True, 13),
                             (1 << 18, 128, False, 13), (1 << 16, 32, False, 11), (1 << 16, 32, True, 17), (1 << 16, 16, False, 9),
                             (1 << 20, 1, False, 3), (1 << 20, 4, True, 5), (1 << 12, 64, True, 8), (1 << 12, 64, False, 5), (20, 8, True, 3)):
        assert msm_pkg.auto_window_size_bounded(n, bits, lone) == c, (n, bits, lone)
    for n in (1, 31, 32, 1 << 12, 1 << 16, 1 << 20, 1 << 22):   # every bounded window is one the pipeline takes
        for bits in (1, 8, 16, 32, 64, 128, 200):
            for lone in (False, True):
                assert 3 <= msm_pkg.auto_window_size_bounded(n, bits, lone) <= 17
