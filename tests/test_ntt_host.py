"""The host twin of the transform (msm_amd_host_ntt: the bodies of csrc/ntt.hip.h compiled for the CPU) against the
big-integer model of tests/ntt_ref.py.  Every comparison is of bytes: outputs are fully reduced, so they are unique."""
import random

import pytest

import ntt_ref as m

R = m.R
SHIFTS = ("none", "five", "random")


def shift_value(kind, seed=0):
    return {"none": None, "five": 5}.get(kind, random.Random(900 + seed).randrange(1, R))


def twin(msm_pkg, values, root, log_n, direction, layout, g=None, n_vec=1, threads=0):
    return msm_pkg.host_ntt(m.encode(values, layout), root, log_n, direction, layout, m.shift_record(g, layout), n_vec,
                            threads)


# ---- 1. roots ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("root", m.ROOTS)
def test_literals_are_g_to_the_t(root):
    assert m.RHO_LITERAL[root] == m.rho(root) == pow(m.GENERATOR[root], (R - 1) >> 28, R)
    assert pow(m.rho(root), 1 << 27, R) == R - 1


@pytest.mark.parametrize("root", m.ROOTS)
def test_forward_of_e1_is_the_powers_of_omega(msm_pkg, root):
    for log_n in range(17):
        n = 1 << log_n
        w = m.omega(root, log_n)
        if log_n >= 1:
            assert pow(w, n // 2, R) == R - 1
        e1 = [0, 1] + [0] * (n - 2) if n > 1 else [1]   # n = 1: the only unit vector
        exp, t = [], 1
        for _ in range(n):
            exp.append(t)
            t = t * w % R
        if n == 1:
            exp = [1]
        assert twin(msm_pkg, e1, root, log_n, m.FORWARD, m.CANON_LE) == m.encode(exp, m.CANON_LE), log_n


# ---- 2. the twin against the definition -------------------------------------------------------------------------------
@pytest.mark.parametrize("root", m.ROOTS)
@pytest.mark.parametrize("direction", m.DIRECTIONS)
@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("shift", SHIFTS)
def test_twin_against_the_naive_dft(msm_pkg, root, direction, layout, shift):
    for log_n in range(7):
        n = 1 << log_n
        g = shift_value(shift, log_n)
        for n_vec in (1, 3):
            vecs = [m.random_vector(1000 * log_n + 10 * n_vec + v, n) for v in range(n_vec)]
            exp = [x for a in vecs for x in m.naive(a, root, log_n, direction, g or 1)]
            got = twin(msm_pkg, [x for a in vecs for x in a], root, log_n, direction, layout, g, n_vec)
            assert got == m.encode(exp, layout), (log_n, n_vec)


# ---- 3. the twin against the radix-2 model ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(7, 14))
def test_twin_against_the_radix2_model(msm_pkg, log_n):
    a = m.random_vector(log_n, 1 << log_n)
    root, direction, layout = log_n & 1, (log_n >> 1) & 1, log_n % 3 == 0
    g = shift_value("random", log_n)
    for r, d, l, gg in ((root, direction, int(layout), g), (1 - root, 1 - direction, 1 - int(layout), None)):
        assert twin(msm_pkg, a, r, log_n, d, l, gg) == m.encode(m.transform(a, r, log_n, d, gg or 1), l), (r, d, l)


def test_model_agrees_with_itself():
    a = m.random_vector(77, 64)
    for root in m.ROOTS:
        for d in m.DIRECTIONS:
            assert m.transform(a, root, 6, d, 11) == m.naive(a, root, 6, d, 11)
    terms = [(1, 5), (35, 7), (63, 9)]
    dense = [0] * 64
    for i, c in terms:
        dense[i] = c
    assert m.naive(dense, m.ARK, 6, m.FORWARD, 3) == [m.sparse_forward(terms, m.ARK, 6, k, 3) for k in range(64)]


# ---- 4. identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_inverse_of_forward_is_the_input(msm_pkg, layout):
    for log_n in (0, 1, 5, 12):
        a = m.encode(m.random_vector(40 + log_n, 2 << log_n), layout)
        for g in (None, 5, shift_value("random")):
            s = m.shift_record(g, layout)
            f = msm_pkg.host_ntt(a, m.H2C, log_n, m.FORWARD, layout, s, 2)
            assert msm_pkg.host_ntt(f, m.H2C, log_n, m.INVERSE, layout, s, 2) == a
            assert f != a or log_n == 0


def test_forward_of_a_constant_polynomial_is_constant(msm_pkg):
    for log_n in (0, 3, 11):
        n = 1 << log_n
        c = 0x1234567890ABCDEF % R
        assert twin(msm_pkg, [c] + [0] * (n - 1), m.ARK, log_n, m.FORWARD, m.MONT_LE, 7) == m.encode([c] * n, m.MONT_LE)


def test_thread_count_changes_nothing(msm_pkg):
    a = m.random_vector(5, 3 << 9)
    assert twin(msm_pkg, a, m.ARK, 9, m.FORWARD, m.MONT_LE, 5, 3, threads=1) == twin(msm_pkg, a, m.ARK, 9, m.FORWARD, m.MONT_LE, 5, 3, threads=7)


# ---- 5. reduction ---------------------------------------------------------------------------------------------------------
def test_inputs_are_read_mod_r_and_outputs_are_reduced(msm_pkg):
    a = [R, R + 1, (1 << 256) - 1, 5 * R + 3, R - 1, 0, 1, 2]
    for direction in m.DIRECTIONS:
        exp = m.transform(a, m.H2C, 3, direction, 5)
        got = msm_pkg.host_ntt(m.encode(a, m.CANON_LE), m.H2C, 3, direction, m.CANON_LE, m.shift_record(5, m.CANON_LE))
        assert got == m.encode(exp, m.CANON_LE)
        assert all(v < R for v in m.decode(got, m.CANON_LE))
        # the same residues through MONT_LE: to_mont of the canonical output; raw Montgomery records >= r are read mod r
        mont = msm_pkg.host_ntt(m.encode(a, m.MONT_LE), m.H2C, 3, direction, m.MONT_LE, m.shift_record(5, m.MONT_LE))
        assert mont == m.encode(exp, m.MONT_LE)
        assert all(int.from_bytes(mont[i:i + 32], "little") < R for i in range(0, len(mont), 32))
    raw = [R, R + 1, (1 << 256) - 1, 7]                       # MONT_LE records taken as they are: x R^-1 mod r
    inv = pow(m.MONT, -1, R)
    got = msm_pkg.host_ntt(b"".join(v.to_bytes(32, "little") for v in raw), m.ARK, 2, m.FORWARD, m.MONT_LE)
    assert got == m.encode(m.naive([v * inv % R for v in raw], m.ARK, 2, m.FORWARD), m.MONT_LE)
    # a shift >= r is reduced like an input
    assert (twin(msm_pkg, a, m.ARK, 3, m.FORWARD, m.CANON_LE, R + 5) == twin(msm_pkg, a, m.ARK, 3, m.FORWARD, m.CANON_LE, 5))


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    import ctypes
    L = msm_pkg.lib()
    n = 8
    data = m.encode(list(range(n)), m.CANON_LE)
    out = ctypes.create_string_buffer(b"\xA5" * (32 * n), 32 * n)
    zero, r_rec = bytes(32), m.encode([R], m.CANON_LE)

    def call(root=0, log_n=3, direction=0, layout=1, shift=None, src=data, dst=out, n_vec=1):
        return L.msm_amd_host_ntt(root, log_n, direction, layout, shift, src, dst, n_vec, 1)

    bad = msm_pkg.INPUT_ERROR
    assert call(root=2) == bad and call(root=-1) == bad
    assert call(direction=2) == bad and call(direction=-1) == bad
    assert call(layout=msm_pkg.SCALAR_CANON_BE32) == bad and call(layout=3) == bad
    assert call(log_n=29, n_vec=0) == bad
    assert call(src=None) == bad and call(dst=None) == bad
    assert call(shift=zero) == bad and call(shift=r_rec) == bad           # g = 0 mod r
    assert call(shift=zero, layout=0) == bad
    assert call(log_n=28, n_vec=16) == bad and call(log_n=3, n_vec=1 << 29) == bad   # n_vec n >= 2^32
    assert call(log_n=0, n_vec=1 << 32) == bad
    assert out.raw == b"\xA5" * (32 * n)                                      # no refused call wrote anything
    assert call(n_vec=0) == msm_pkg.OK and call(n_vec=0, src=None, dst=None) == msm_pkg.OK
    assert out.raw == b"\xA5" * (32 * n)                                      # n_vec = 0 touches nothing
    assert call() == msm_pkg.OK and out.raw == m.encode(m.naive(list(range(n)), 0, 3, 0), m.CANON_LE)
