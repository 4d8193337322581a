"""The host twins of the Fr vector calls (msm_amd_host_fr_map, msm_amd_host_fr_batch_inverse,
msm_amd_host_fr_prefix_product: the bodies of csrc/fr_vec.hip.h compiled for the CPU) against the big-integer model of
tests/fr_ref.py, and the plan of the device scan (msm_amd_test_fr_plan).  Every comparison is of bytes: outputs are fully
reduced, so they are unique."""
import ctypes
import random

import pytest

import fr_ref as m

R = m.R
SIZES = (1, 2, 3, 63, 64, 65, 1000)
T = 9    # the default tile of the scan, as a power of two


def operands(seed, n, layout):
    return [m.encode(m.random_values(seed + j, n), layout) for j in range(3)]


def k_record(seed, layout):
    return m.encode([random.Random(seed).randrange(1, R)], layout)


# ---- 1. the twins against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("op", m.OPS)
def test_map_matches_the_model(msm_pkg, op, layout):
    for n in SIZES:
        a, b, c = operands(10 * n, n, layout)
        k = k_record(n, layout)
        exp = m.fr_map(op, layout, a, b, c, k)
        assert m.first_difference(msm_pkg.host_fr_map(op, a, b, c, k, layout), exp) is None, n
        assert msm_pkg.host_fr_map(op, a, b, c, k, layout, threads=1) == msm_pkg.host_fr_map(op, a, b, c, k, layout, threads=16)


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_map_ignores_what_the_op_does_not_read(msm_pkg, layout):
    a, b, c = operands(5, 7, layout)
    k = k_record(5, layout)
    assert msm_pkg.host_fr_map(m.ADD, a, b, None, None, layout) == m.fr_map(m.ADD, layout, a, b)
    assert msm_pkg.host_fr_map(m.SCALE, a, None, None, k, layout) == m.fr_map(m.SCALE, layout, a, k=k)
    assert msm_pkg.host_fr_map(m.AXPY, a, b, None, k, layout) == m.fr_map(m.AXPY, layout, a, b, k=k)
    assert msm_pkg.host_fr_map(m.MUL, a, a, None, None, layout) == m.encode([x * x for x in m.decode(a, layout)], layout)


@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("op", m.OPS)
def test_unreduced_inputs_and_k(msm_pkg, op, layout):
    """any 256-bit word is a residue: r, r + 1, 2^256 - 1 ... as operands and as k"""
    a = m.raw(m.UNREDUCED)
    b = m.raw(m.UNREDUCED[::-1])
    c = m.raw(m.UNREDUCED[2:] + m.UNREDUCED[:2])
    for kw in m.UNREDUCED:
        k = m.raw([kw])
        exp = m.fr_map(op, layout, a, b, c, k)
        assert m.words(exp) == [w % R for w in m.words(exp)]
        assert m.first_difference(msm_pkg.host_fr_map(op, a, b, c, k, layout), exp) is None, kw
    assert msm_pkg.host_fr_batch_inverse(a, layout) == m.batch_inverse(a, layout)
    assert m.batch_inverse(a, layout)[1] == 1   # the word r is zero in both layouts
    for mode in m.MODES:
        assert msm_pkg.host_fr_prefix_product(a[32:] * 3, mode, layout) == m.prefix_product(a[32:] * 3, layout, mode)


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_minus_one_everywhere(msm_pkg, layout):
    """r - 1 in every record: products alternate between -1 and 1"""
    n = 67
    data = m.encode([R - 1] * n, layout)
    inc = msm_pkg.host_fr_prefix_product(data, m.INCLUSIVE, layout)
    assert inc == m.encode([R - 1 if i % 2 == 0 else 1 for i in range(n)], layout)
    exc = msm_pkg.host_fr_prefix_product(data, m.EXCLUSIVE, layout)
    assert exc == m.encode([1 if i % 2 == 0 else R - 1 for i in range(n)], layout)
    assert msm_pkg.host_fr_batch_inverse(data, layout) == (data, 0)
    assert msm_pkg.host_fr_map(m.MUL, data, data, None, None, layout) == m.encode([1] * n, layout)
    assert msm_pkg.host_fr_map(m.ADD, data, data, None, None, layout) == m.encode([R - 2] * n, layout)
    assert msm_pkg.host_fr_map(m.MULSUB_SCALE, data, data, data, data[:32], layout) == m.encode([R - 2] * n, layout)


def zero_patterns(n):
    pats = {"none": [], "first": [0], "last": [n - 1], "all": list(range(n))}
    if n >= 3:
        pats["adjacent"] = [n // 2, n // 2 + 1]
        pats["ends"] = [0, n - 1]
    return pats


@pytest.mark.parametrize("layout", m.LAYOUTS)
def test_inverse_with_zeros(msm_pkg, layout):
    for n in SIZES:
        for name, zeros in zero_patterns(n).items():
            vals = m.random_values(40 + n, n)
            for i in zeros:
                vals[i] = 0
            data = m.encode(vals, layout)
            exp, n_zero = m.batch_inverse(data, layout)
            assert n_zero == len(set(zeros))
            for threads in (1, 16):
                got, got_zero = msm_pkg.host_fr_batch_inverse(data, layout, threads)
                assert m.first_difference(got, exp) is None, (n, name, threads)
                assert got_zero == n_zero, (n, name, threads)


@pytest.mark.parametrize("layout", m.LAYOUTS)
@pytest.mark.parametrize("mode", m.MODES)
def test_prefix_products(msm_pkg, mode, layout):
    for n in SIZES:
        for n_vec in (1, 3):
            data = m.encode(m.random_values(70 + n + n_vec, n * n_vec), layout)
            exp = m.prefix_product(data, layout, mode, n_vec)
            one, many = (msm_pkg.host_fr_prefix_product(data, mode, layout, n_vec, threads) for threads in (1, 16))
            assert m.first_difference(one, exp) is None, (n, n_vec)
            assert many == one, (n, n_vec)
            if n_vec == 3:   # the product restarts: every vector alone gives the same records
                alone = b"".join(msm_pkg.host_fr_prefix_product(data[32 * n * v:32 * n * (v + 1)], mode, layout)
                                 for v in range(3))
                assert alone == one


def test_prefix_with_a_zero_stays_zero(msm_pkg):
    vals = m.random_values(3, 40)
    vals[17] = 0
    data = m.encode(vals, m.MONT_LE)
    out = m.decode(msm_pkg.host_fr_prefix_product(data, m.INCLUSIVE, m.MONT_LE), m.MONT_LE)
    assert all(out[:17]) and not any(out[17:])


# ---- 2. in place -------------------------------------------------------------------------------------------------------------
def test_in_place(msm_pkg):
    L, n, layout = msm_pkg.lib(), 65, m.CANON_LE
    a, b, c = operands(91, n, layout)
    k = k_record(91, layout)
    for op in m.OPS:
        exp = m.fr_map(op, layout, a, b, c, k)
        for target in range(3):
            if "abc"[target] not in m.READS[op]:
                continue
            bufs = [ctypes.create_string_buffer(x, len(x)) for x in (a, b, c)]
            assert L.msm_amd_host_fr_map(op, layout, k, bufs[0], bufs[1], bufs[2], n, 0, bufs[target]) == msm_pkg.OK
            assert bufs[target].raw == exp, (op, target)
            for other in range(3):
                if other != target:
                    assert bufs[other].raw == (a, b, c)[other]
    buf = ctypes.create_string_buffer(a, len(a))
    assert L.msm_amd_host_fr_map(m.MUL, layout, None, buf, buf, None, n, 0, buf) == msm_pkg.OK       # a == b == out
    assert buf.raw == m.fr_map(m.MUL, layout, a, a)
    vals = m.random_values(92, n)
    vals[0] = vals[n - 1] = 0
    data = m.encode(vals, layout)
    buf, zeros = ctypes.create_string_buffer(data, len(data)), ctypes.c_uint64(99)
    assert L.msm_amd_host_fr_batch_inverse(layout, buf, n, 0, buf, ctypes.byref(zeros)) == msm_pkg.OK
    assert (buf.raw, zeros.value) == m.batch_inverse(data, layout)
    for mode in m.MODES:
        buf = ctypes.create_string_buffer(data[32:32 * 61], 32 * 60)
        assert L.msm_amd_host_fr_prefix_product(layout, mode, buf, 20, 3, 0, buf) == msm_pkg.OK
        assert buf.raw == m.prefix_product(data[32:32 * 61], layout, mode, 3)


# ---- 3. arguments --------------------------------------------------------------------------------------------------------------
def test_input_errors_and_empty_calls(msm_pkg):
    L, n = msm_pkg.lib(), 8
    a, b, c = operands(1, n, m.MONT_LE)
    k = k_record(1, m.MONT_LE)
    big = ctypes.create_string_buffer(a + b, 64 * n)
    base = ctypes.addressof(big)
    out = ctypes.create_string_buffer(b"\xA5" * (32 * n), 32 * n)
    zeros = ctypes.c_uint64(77)
    vp = ctypes.c_void_p

    def status(fn, *args):
        return fn(*args)

    bad = msm_pkg.INPUT_ERROR
    fmap, finv, fpre = L.msm_amd_host_fr_map, L.msm_amd_host_fr_batch_inverse, L.msm_amd_host_fr_prefix_product
    assert status(fmap, 6, 0, k, a, b, c, n, 0, out) == bad                       # unknown op
    assert status(fmap, -1, 0, k, a, b, c, n, 0, out) == bad
    assert status(fmap, m.ADD, m.CANON_BE32, k, a, b, c, n, 0, out) == bad        # layout
    assert status(fmap, m.ADD, 3, k, a, b, c, n, 0, out) == bad
    assert status(fmap, m.ADD, 0, k, None, b, c, n, 0, out) == bad                # a null operand that is read
    assert status(fmap, m.ADD, 0, k, a, None, c, n, 0, out) == bad
    assert status(fmap, m.MULSUB_SCALE, 0, k, a, b, None, n, 0, out) == bad
    assert status(fmap, m.SCALE, 0, None, a, b, c, n, 0, out) == bad              # k is read
    assert status(fmap, m.ADD, 0, k, a, b, c, n, 0, None) == bad
    assert status(fmap, m.ADD, 0, k, a, b, c, 1 << 32, 0, out) == bad
    assert status(fmap, m.ADD, 0, k, vp(base), vp(base + 32 * n), None, n, 0, vp(base + 32)) == bad      # partial overlap with a
    assert status(fmap, m.ADD, 0, k, vp(base), vp(base + 32 * n), None, n, 0, vp(base + 32 * n - 32)) == bad   # ... with both
    assert status(fmap, m.SCALE, 0, k, vp(base + 32), None, None, n, 0, vp(base)) == bad
    assert status(finv, m.CANON_BE32, a, n, 0, out, ctypes.byref(zeros)) == bad and zeros.value == 0
    assert status(finv, 0, None, n, 0, out, None) == bad
    assert status(finv, 0, a, n, 0, None, None) == bad
    assert status(finv, 0, a, 1 << 32, 0, out, None) == bad
    assert status(finv, 0, vp(base), n, 0, vp(base + 32), None) == bad
    assert status(fpre, 0, 2, a, n, 1, 0, out) == bad                             # mode
    assert status(fpre, m.CANON_BE32, 0, a, n, 1, 0, out) == bad
    assert status(fpre, 0, 0, None, n, 1, 0, out) == bad
    assert status(fpre, 0, 0, a, n, 1, 0, None) == bad
    assert status(fpre, 0, 0, a, 1 << 16, 1 << 16, 0, out) == bad                 # n n_vec = 2^32
    assert status(fpre, 0, 0, vp(base), n, 1, 0, vp(base + 32)) == bad
    assert out.raw == b"\xA5" * (32 * n) and big.raw == a + b
    # nothing to do: OK, nothing touched, null pointers allowed
    zeros.value = 77
    assert status(fmap, m.ADD, 0, None, None, None, None, 0, 0, None) == msm_pkg.OK
    assert status(finv, 0, None, 0, 0, None, ctypes.byref(zeros)) == msm_pkg.OK and zeros.value == 0
    assert status(fpre, 0, 0, None, 0, 3, 0, None) == msm_pkg.OK
    assert status(fpre, 0, 0, None, 3, 0, 0, None) == msm_pkg.OK
    assert out.raw == b"\xA5" * (32 * n)
    # operands the op does not read may be anything, also overlapping the output
    assert status(fmap, m.SCALE, 0, k, vp(base), vp(base + 32), vp(base + 64), n, 0, vp(base)) == msm_pkg.OK
    assert big.raw == m.fr_map(m.SCALE, 0, a, k=k) + b


# ---- 4. the plan of the device scan ------------------------------------------------------------------------------------------
def test_plan_levels_launches_memory(msm_pkg):
    plan = msm_pkg.test_fr_plan
    for t in (2, 3, T):
        tile = 1 << t
        for n, levels in ((1, 1), (tile - 1, 1), (tile, 1), (tile + 1, 2), (tile * tile, 2), (tile * tile + 1, 3),
                          (tile ** 3, 3), (tile ** 3 + 1, 4)):
            for n_vec in (1, 3):
                if n * n_vec >= 1 << 32:
                    continue
                p = plan(n, n_vec, t)
                assert p["levels"] == levels, (t, n)
                assert p["launches"] == 2 * levels - 1
                assert p["tiles"] == -(-n // tile) * n_vec
                records, length = 0, n
                for _ in range(levels - 1):   # every level above the first holds one record per tile of the one below
                    length = -(-length // tile)
                    records += length * n_vec
                assert p["records"] == records, (t, n, n_vec)
    assert plan(257, 1, 2)["levels"] == 5 and plan(513, 2, 2)["levels"] == 5 and plan(70, 1, 3)["levels"] == 3
    assert plan(0, 1, T) == plan(5, 0, T) == {"levels": 0, "launches": 0, "tiles": 0, "records": 0}
    for bad in ((1 << 32, 1, T), (1 << 16, 1 << 16, T), (5, 1, 1), (5, 1, T + 1)):
        with pytest.raises(msm_pkg.MsmError) as e:
            plan(*bad)
        assert e.value.status == msm_pkg.INPUT_ERROR
