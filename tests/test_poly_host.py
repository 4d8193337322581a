"""The host twins of the polynomial calls (msm_amd_host_fr_poly_eval, msm_amd_host_fr_poly_div_linear,
msm_amd_host_fr_lincomb) against the big-integer model of tests/poly_ref.py.  No GPU.  Every comparison is of bytes: the
records of a result are unique."""
import ctypes
import random

import pytest

import poly_ref as m

R = m.R
SIZES = list(range(1, 71)) + [257, 513]


def coefficient_patterns(n, seed):
    """(name, records as raw 256-bit words) -- the layout decides what a word means"""
    rng = random.Random(seed)
    unreduced = (R, R + 1, (1 << 256) - 1, 2 * R - 1, 5 * R + 7)
    return {
        "random": [rng.randrange(R) for _ in range(n)],
        "zero": [0] * n,
        "minus_one": None,                                 # r - 1 as a value: encoded per layout
        "unreduced": [unreduced[i % 5] for i in range(n)],
        "first": [rng.randrange(1, R)] + [0] * (n - 1),
        "last": [0] * (n - 1) + [rng.randrange(1, R)],
    }


def records(name, words, n, layout):
    if name == "minus_one":
        return m.encode([R - 1] * n, layout)
    if name == "unreduced":
        return m.raw(words)
    return m.encode(words, layout)


def check_all(msm_pkg, data, z, layout, n_vec, tag):
    exp_y = m.poly_eval(data, z, layout, n_vec)
    exp_q, exp_rem = m.div_linear(data, z, layout, n_vec)
    assert exp_rem == exp_y, tag
    for threads in (1, 16):
        assert msm_pkg.host_fr_poly_eval(data, z, layout, n_vec, threads) == exp_y, (tag, threads)
        q, rem = msm_pkg.host_fr_poly_div_linear(data, z, layout, n_vec, threads)
        assert m.first_difference(q, exp_q) is None, (tag, threads)
        assert rem == exp_rem, (tag, threads)
        assert msm_pkg.host_fr_lincomb(data, z, layout, n_vec, threads) == m.lincomb(data, z, layout, n_vec), (tag, threads)


# ---- 1. the twins against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("n_vec", [1, 3])
def test_every_size_and_point(msm_pkg, layout, n_vec):
    points = m.special_points(layout)
    for n in SIZES:
        data = m.encode(m.random_values(11 * n + n_vec, n * n_vec), layout)
        # every point at the sizes where a range of a thread, a vector and a word boundary meet; two of them elsewhere
        chosen = points if n <= 20 or n in (64, 65, 257, 513) else (points[n % 6], points[6])
        for name, z in chosen:
            check_all(msm_pkg, data, z, layout, n_vec, (n, name))


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_coefficient_patterns(msm_pkg, layout):
    points = m.special_points(layout)
    for n in (1, 2, 17, 64, 70, 257):
        for name, words in coefficient_patterns(n, n).items():
            data = records(name, words, n, layout)
            for pname, z in points:
                check_all(msm_pkg, data, z, layout, 1, (n, name, pname))
            check_all(msm_pkg, data * 3, points[6][1], layout, 3, (n, name, "three"))


def test_vectors_restart(msm_pkg):
    """three polynomials in one call give what each gives alone"""
    layout, z = m.MONT_LE, m.special_points(m.MONT_LE)[6][1]
    for n in (1, 5, 33, 70):
        data = m.encode(m.random_values(5 + n, 3 * n), layout)
        alone = [msm_pkg.host_fr_poly_div_linear(data[32 * n * v:32 * n * (v + 1)], z, layout) for v in range(3)]
        q, rem = msm_pkg.host_fr_poly_div_linear(data, z, layout, 3)
        assert q == b"".join(a[0] for a in alone) and rem == b"".join(a[1] for a in alone)
        assert msm_pkg.host_fr_poly_eval(data, z, layout, 3) == rem


def test_threads_change_nothing(msm_pkg):
    layout = m.CANON_LE
    z = m.special_points(layout)[6][1]
    for n, n_vec in ((1, 40), (3, 11), (37, 3), (513, 1), (1000, 2)):
        data = m.encode(m.random_values(n, n * n_vec), layout)
        base = (msm_pkg.host_fr_poly_eval(data, z, layout, n_vec, 1), msm_pkg.host_fr_poly_div_linear(data, z, layout, n_vec, 1),
                msm_pkg.host_fr_lincomb(data, z, layout, n_vec, 1))
        assert base[0] == m.poly_eval(data, z, layout, n_vec) and base[1] == m.div_linear(data, z, layout, n_vec)
        for threads in (2, 3, 7, 16):
            got = (msm_pkg.host_fr_poly_eval(data, z, layout, n_vec, threads),
                   msm_pkg.host_fr_poly_div_linear(data, z, layout, n_vec, threads),
                   msm_pkg.host_fr_lincomb(data, z, layout, n_vec, threads))
            assert got == base, (n, n_vec, threads)


# ---- 2. in place ---------------------------------------------------------------------------------------------------------------
def test_in_place(msm_pkg):
    L, layout = msm_pkg.lib(), m.MONT_LE
    z = m.special_points(layout)[6][1]
    for n, n_vec in ((1, 1), (65, 1), (40, 3)):
        data = m.encode(m.random_values(90 + n, n * n_vec), layout)
        exp_q, exp_rem = m.div_linear(data, z, layout, n_vec)
        buf = ctypes.create_string_buffer(data, len(data))
        rem = ctypes.create_string_buffer(32 * n_vec)
        assert L.msm_amd_host_fr_poly_div_linear(layout, z, buf, n, n_vec, 0, buf, rem) == msm_pkg.OK
        assert buf.raw == exp_q and rem.raw == exp_rem
        src, out = ctypes.create_string_buffer(data, len(data)), ctypes.create_string_buffer(b"\xFF" * len(data), len(data))
        assert L.msm_amd_host_fr_poly_div_linear(layout, z, src, n, n_vec, 0, out, None) == msm_pkg.OK    # no remainder asked for
        assert out.raw == exp_q and src.raw == data
        buf = ctypes.create_string_buffer(data, len(data))
        assert L.msm_amd_host_fr_lincomb(layout, z, buf, n, n_vec, 0, buf) == msm_pkg.OK                  # onto vector 0
        assert buf.raw == m.lincomb(data, z, layout, n_vec) + data[32 * n:]


# ---- 3. identities on model integers -------------------------------------------------------------------------------------------
def test_identities():
    rng = random.Random(12)
    for n in (1, 2, 9, 64, 130):
        c = [rng.randrange(R) for _ in range(n)]
        z, tau = rng.randrange(R), rng.randrange(R)
        q, rem = m.div_linear_definition(c, z)
        assert (q, rem) == tuple(m.div_linear_horner(c, z))
        assert (m.eval_ints(q, tau) * (tau - z) + rem) % R == m.eval_ints(c, tau)
        assert rem == m.eval_ints(c, z) and q[n - 1] == 0
        q0, rem0 = m.div_linear_definition(c, 0)
        assert q0 == c[1:] + [0] and rem0 == c[0]


def test_identities_of_the_twins(msm_pkg):
    layout = m.MONT_LE
    n = 70
    words = [((3 * i + 1) * R // 7 + i) % (1 << 256) for i in range(n)]   # 256-bit words on both sides of r
    data = m.raw(words)
    k = m.special_points(layout)[6][1]
    assert msm_pkg.host_fr_lincomb(data, k, layout, 1) == m.encode(m.decode(data, layout), layout)     # the reduced copy
    zero = m.point_record(0, layout)
    q, rem = msm_pkg.host_fr_poly_div_linear(data, zero, layout)
    reduced = m.encode(m.decode(data, layout), layout)
    assert q == reduced[32:] + bytes(32) and rem == reduced[:32]
    rng = random.Random(4)
    z, tau = rng.randrange(R), rng.randrange(R)
    q, rem = msm_pkg.host_fr_poly_div_linear(data, m.encode([z], layout), layout)
    qi, ri, ci = m.decode(q, layout), m.decode(rem, layout)[0], m.decode(data, layout)
    assert (m.eval_ints(qi, tau) * (tau - z) + ri) % R == m.eval_ints(ci, tau)


# ---- 4. arguments ----------------------------------------------------------------------------------------------------------------
def test_input_errors_and_empty_calls(msm_pkg):
    L, n = msm_pkg.lib(), 8
    a = m.encode(m.random_values(1, 3 * n), m.MONT_LE)
    z = m.encode([5], m.MONT_LE)
    big = ctypes.create_string_buffer(a + a, 2 * len(a))
    base = ctypes.addressof(big)
    out = ctypes.create_string_buffer(b"\xA5" * len(a), len(a))
    y = ctypes.create_string_buffer(b"\xA5" * 96, 96)
    vp = ctypes.c_void_p
    bad, ok = msm_pkg.INPUT_ERROR, msm_pkg.OK
    fev, fdiv, flc = L.msm_amd_host_fr_poly_eval, L.msm_amd_host_fr_poly_div_linear, L.msm_amd_host_fr_lincomb
    for layout in (msm_pkg.SCALAR_CANON_BE32, 3, -1):                                   # CANON_BE32 and unknown layouts
        assert fev(layout, z, a, n, 3, 0, y) == bad
        assert fdiv(layout, z, a, n, 3, 0, out, y) == bad
        assert flc(layout, z, a, n, 3, 0, out) == bad
    assert fev(0, None, a, n, 3, 0, y) == bad                                  # null pointers
    assert fev(0, z, None, n, 3, 0, y) == bad
    assert fev(0, z, a, n, 3, 0, None) == bad
    assert fdiv(0, None, a, n, 3, 0, out, y) == bad
    assert fdiv(0, z, None, n, 3, 0, out, y) == bad
    assert fdiv(0, z, a, n, 3, 0, None, y) == bad
    assert flc(0, None, a, n, 3, 0, out) == bad
    assert flc(0, z, None, n, 3, 0, out) == bad
    assert flc(0, z, a, n, 3, 0, None) == bad
    assert fev(0, z, a, 1 << 16, 1 << 16, 0, y) == bad                         # n n_vec = 2^32
    assert fdiv(0, z, a, 1 << 32, 1, 0, out, y) == bad
    assert flc(0, z, a, 1, 1 << 32, 0, out) == bad
    assert fdiv(0, z, vp(base), n, 3, 0, vp(base + 32), y) == bad              # partial overlap
    assert fdiv(0, z, vp(base + 32), n, 3, 0, vp(base), y) == bad
    assert flc(0, z, vp(base), n, 3, 0, vp(base + 32)) == bad
    assert flc(0, z, vp(base), n, 3, 0, vp(base + 32 * n)) == bad              # the second vector
    assert flc(0, z, vp(base), n, 3, 0, vp(base + 32 * n * 3 - 32)) == bad     # the last record of a
    assert flc(0, z, vp(base + 32), n, 3, 0, vp(base)) == bad
    assert out.raw == b"\xA5" * len(a) and y.raw == b"\xA5" * 96 and big.raw == a + a
    assert flc(0, z, vp(base), n, 3, 0, vp(base + 32 * n * 3)) == ok           # right behind a: disjoint
    assert big.raw[32 * n * 3:32 * n * 4] == m.lincomb(a, z, m.MONT_LE, 3)
    # nothing to do: OK, nothing touched, null pointers allowed
    for nn, nv in ((0, 3), (3, 0), (0, 0)):
        assert fev(0, None, None, nn, nv, 0, y) == ok
        assert fdiv(0, None, None, nn, nv, 0, out, y) == ok
        assert flc(0, None, None, nn, nv, 0, out) == ok
    assert out.raw == b"\xA5" * len(a) and y.raw == b"\xA5" * 96
    assert msm_pkg.host_fr_poly_eval(b"", z) == b"" and msm_pkg.host_fr_lincomb(b"", z) == b""
    assert msm_pkg.host_fr_poly_div_linear(b"", z) == (b"", b"")
