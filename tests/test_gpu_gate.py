"""The gate polynomials on the GPU (msm_amd_fr_gate_eval; host and device memory) against the host twin and the big-integer
model of tests/gate_ref.py (tests/test_gate_host.py pins the twin to the model on the CPU).  Every comparison is of bytes:
device-memory call = host-buffer call = twin = model.  The kernel is one lane per row in workgroups of 256: the shapes are the
smallest at which it can go wrong -- one and two rows, the wave and workgroup edges, a size that is no power of two, rotations
that wrap in the first and in the last workgroup -- and the structural test runs a PLONK gate through the transforms."""
import random

import pytest

import gate_ref as g
import mle_ref as m

pytestmark = pytest.mark.gpu

R = g.R
POISON = b"\xFF" * 32


class Device:
    """device buffers of one test, freed together"""

    def __init__(self, cfg, pkg):
        self.cfg, self.pkg, self.ptrs = cfg, pkg, []

    def put(self, data):
        d = self.cfg.alloc(max(32, len(data)))
        self.ptrs.append(d)
        self.cfg.to_device(d, data)
        return d

    def get(self, d, nbytes):
        return self.cfg.to_host(d, nbytes)

    def close(self):
        for d in self.ptrs:
            self.cfg.free(d)
        self.ptrs = []


@pytest.fixture
def dev(cfg, msm_pkg):
    d = Device(cfg, msm_pkg)
    yield d
    d.close()


def device_eval(dev, terms, data, n, n_vec, stride, rot_step, layout, old=None, **kw):
    """a call on fresh device buffers, out poisoned (or holding `old`) with three records behind it: the n records; the
    input and the records behind out must survive"""
    d_in = dev.put(data)
    d_out = dev.put((old if old is not None else POISON * n) + POISON * 3)
    _, ms = dev.cfg.fr_gate_eval(d_in, terms, n, n_vec, stride, rot_step, out=d_out, scalar_layout=layout, mem=dev.pkg.MEM_DEVICE, **kw)
    assert ms >= 0 and dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, 32 * (n + 3))
    dev.close()
    assert out[32 * n:] == POISON * 3, "wrote behind out"
    return out[:32 * n]


def check_gate(cfg, dev, gate, n, layout, seed, stride=None, edge=False, model=True):
    """plain into poison: device = host-buffer call = twin (= model)"""
    pkg = dev.pkg
    stride = n if stride is None else stride
    tag = (gate, n, layout)
    terms = gate.lib_terms(pkg, layout)
    data = g.columns(seed, n, gate.n_vec, layout, stride, edge)
    twin = pkg.host_fr_gate_eval(data, terms, n, gate.n_vec, stride, gate.rot_step, scalar_layout=layout, threads=16, out=POISON * n)
    if model:
        assert twin == g.evaluate(data, layout, gate, n, stride), tag
    assert POISON not in [twin[i:i + 32] for i in range(0, len(twin), 32)], tag
    assert device_eval(dev, terms, data, n, gate.n_vec, stride, gate.rot_step, layout) == twin, tag
    got, _ = cfg.fr_gate_eval(data, terms, n, gate.n_vec, stride, gate.rot_step, out=POISON * n, scalar_layout=layout)
    assert got == twin, tag


# ---- 1. every gate of the issue at every edge size ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", g.SIZES)
def test_sizes_rotations_and_coefficients(cfg, dev, n):
    """n = 1 (every rotation lands on the row itself), 2, the wave and workgroup edges, 1000; rotations -1 and +1 wrap rows 0
    and n - 1 (at 257 and 1000 in the first and in the last workgroup); far rotations, one that is 0 mod n at n = 1000,
    INT32_MIN at rot_step 2^40; eight offsets; a copy, an eighth power, sixteen terms; coefficients 1, r - 1, 0, raw words
    and random; records >= r in CANON_LE; both layouts; stride n + 5"""
    for layout in g.LAYOUTS:
        for j, gate in enumerate(g.GATES):
            check_gate(cfg, dev, gate, n, layout, 100 * n + j, stride=n + 5 * (j & 1), edge=layout == g.CANON_LE and j % 2 == 0)


def test_wrapped_rows_in_the_first_and_last_workgroup(cfg, dev):
    """three workgroups: row 0 reads row n - 1 (the last workgroup's) and row n - 1 reads row 0, spelled out by hand"""
    n, layout, gate = 600, g.MONT_LE, g.Gate("shifted", 1, [(1, [(0, -1)]), (1, [(0, 1)])])
    data = g.columns(600, n, 1, layout)
    v = m.decode(data, layout)
    out = device_eval(dev, gate.lib_terms(dev.pkg, layout), data, n, 1, n, 1, layout)
    assert out == m.encode([(v[i - 1] + v[(i + 1) % n]) % R for i in range(n)], layout)


def test_eight_offsets_exactly_and_nine_refused(cfg, dev):
    pkg = dev.pkg
    n, layout = 257, g.MONT_LE
    assert pkg.fr_gate_check(g.EIGHT_OFFSETS.lib_terms(pkg, layout), 3, n) == (4, pkg.GATE_MAX_OFFSETS)
    check_gate(cfg, dev, g.EIGHT_OFFSETS, n, layout, 8)
    nine = g.Gate("nine", 2, [(1, [(0, r) for r in range(5)]), (1, [(1, r) for r in range(5, 9)])])
    with pytest.raises(pkg.MsmError, match=r"msm_amd_fr_gate_eval: more than MSM_AMD_GATE_MAX_OFFSETS \(8\) distinct offsets"):
        cfg.fr_gate_eval(g.columns(9, n, 2, layout), nine.lib_terms(pkg, layout), n, 2)
    check_gate(cfg, dev, nine, 8, layout, 9)   # the same rotations are eight offsets at n = 8


def test_column_255_of_256(cfg, dev):
    gate = g.Gate("last-column", 256, [(1, [(255, 1), 0]), (R - 1, [(255, -1)])])
    for layout in g.LAYOUTS:
        check_gate(cfg, dev, gate, 4, layout, 255, stride=9)


# ---- 2. accumulate and scale --------------------------------------------------------------------------------------------------
def test_accumulate_chained_over_three_calls(cfg, dev):
    """three gates folded by y as halo2 folds them, ((g0) y + g1) y + g2, against ONE big-integer evaluation; device memory and
    host buffers"""
    pkg = dev.pkg
    n, layout = 257, g.CANON_LE
    gates = (g.NEIGHBOURS, g.Gate("b", 2, [(3, [(1, 2), 1])]), g.Gate("c", 2, [(R - 1, [0]), (1, [(1, -1)])]))
    data = g.columns(77, n, 2, layout, edge=True)
    y = m.raw([R + 5])                                        # a challenge word >= r
    cols, yy = m.tables(data, layout, n, 2), 5
    v = [g.rows_ints(cols, gate, gate.coeff_values(layout)) for gate in gates]
    expect = m.encode([((a * yy + b) * yy + c) % R for a, b, c in zip(*v)], layout)
    d_in, d_out = dev.put(data), dev.put(POISON * n)
    host = POISON * n
    for k, gate in enumerate(gates):
        terms, flags = gate.lib_terms(pkg, layout), pkg.GATE_ACCUMULATE if k else 0
        cfg.fr_gate_eval(d_in, terms, n, 2, flags=flags, k_acc=y, out=d_out, scalar_layout=layout, mem=pkg.MEM_DEVICE)
        host, _ = cfg.fr_gate_eval(data, terms, n, 2, flags=flags, k_acc=y, out=host, scalar_layout=layout)
    assert dev.get(d_out, 32 * n) == expect and host == expect
    assert dev.get(d_in, len(data)) == data


@pytest.mark.parametrize("n", (256, 1024))
def test_scale_periods_with_and_without_accumulate(cfg, dev, n):
    pkg = dev.pkg
    for layout in g.LAYOUTS:
        gate = g.NEIGHBOURS
        terms = gate.lib_terms(pkg, layout)
        data = g.columns(n, n, gate.n_vec, layout)
        old, k_acc = g.records(1, n, layout), g.records(2, 1, layout)
        for period in (1, 4, 256):
            scale = g.records(3 + period, period, layout)
            for acc in (False, True):
                kw = dict(flags=pkg.GATE_ACCUMULATE, k_acc=k_acc) if acc else {}
                expect = g.evaluate(data, layout, gate, n, scale=scale, **(dict(old=old, k_acc=k_acc) if acc else {}))
                tag = (n, layout, period, acc)
                assert device_eval(dev, terms, data, n, 2, n, 1, layout, old=old if acc else None, scale=scale, **kw) == expect, tag
                got, _ = cfg.fr_gate_eval(data, terms, n, 2, out=old if acc else POISON * n, scalar_layout=layout, scale=scale, **kw)
                assert got == expect, tag
                assert pkg.host_fr_gate_eval(data, terms, n, 2, out=old if acc else POISON * n, scalar_layout=layout, scale=scale,
                                             **kw) == expect, tag


def test_empty_calls_and_refusals_by_text(cfg, dev):
    pkg = dev.pkg
    n, layout = 16, g.MONT_LE
    terms = g.NEIGHBOURS.lib_terms(pkg, layout)
    data = g.columns(1, n, 2, layout)
    d_in, d_out = dev.put(data), dev.put(POISON * n)
    for kw in (dict(n=0, n_vec=2), dict(n=n, n_vec=0)):
        cfg.fr_gate_eval(d_in, None, out=d_out, mem=pkg.MEM_DEVICE, **kw)
        assert dev.get(d_out, 32 * n) == POISON * n
    rec = g.records(1, 512, layout)
    cases = (
        (dict(mem=2), "mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE"),
        (dict(scalar_layout=pkg.SCALAR_CANON_BE32), "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only"),
        (dict(flags=4), "flags must be 0 or MSM_AMD_GATE_ACCUMULATE"),
        (dict(flags=pkg.GATE_ACCUMULATE), "null k_acc32 with MSM_AMD_GATE_ACCUMULATE"),
        (dict(rot_step=0), "rot_step must be at least 1"),
        (dict(stride=n - 1), "stride < n"),
        (dict(scale=rec[:32 * 3]), "period must be a power of two"),
        (dict(scale=rec[:32 * 32]), "period must be a power of two"),
        (dict(scale=rec), "period must be a power of two"),
        (dict(out=d_out + 8), "device buffers must be 16-byte aligned"),
        (dict(out=d_in + 32 * (2 * n - 1)), "the output must be disjoint from all of the input"),
        (dict(out=0), "null pointer with work to do"),
    )
    for kw, text in cases:
        args = dict(n=n, n_vec=2, out=d_out, mem=pkg.MEM_DEVICE)
        args.update(kw)
        with pytest.raises(pkg.MsmError) as e:
            cfg.fr_gate_eval(d_in, terms, **args)
        assert e.value.status == pkg.INPUT_ERROR and "msm_amd_fr_gate_eval: " + text in str(e.value), (kw, str(e.value))
        assert dev.get(d_out, 32 * n) == POISON * n and dev.get(d_in, len(data)) == data, kw


# ---- 3. the structure: a PLONK gate through the transforms ------------------------------------------------------------------------
def test_plonk_quotient_on_the_extended_coset(cfg, dev):
    """8 rows extended by 4.  Columns q_L, q_R, q_M, q_O, q_C, a, b, c with q_L a + q_R b + q_M a b - q_O c(w X) + q_C = 0 on
    H go to the coset g H' of 32 points with msm_amd_ntt_device; the gate call reads c at rotation +1 with rot_step 4 and
    scales by 1 / Z_H (period 4); the inverse coset transform gives h.  Then deg h <= 3 * 7 - 8 = 13, so the top 18
    coefficients are zero -- which fails if rot_step is applied wrongly, the quotient being no polynomial then -- and
    h(x) Z_H(x) equals the gate at a random x through msm_amd_fr_poly_eval_device."""
    pkg = dev.pkg
    layout, k, ext = g.MONT_LE, 3, 2
    n, big = 1 << k, 1 << (k + ext)
    rng = random.Random(0x910C)
    val = lambda: [rng.randrange(R) for _ in range(n)]  # noqa: E731
    ql, qr, qm, qc, a, b = val(), val(), val(), val(), val(), val()
    qo = [rng.randrange(1, R) for _ in range(n)]
    c = [0] * n
    for i in range(n):   # row i reads c at row i + 1
        c[(i + 1) % n] = (ql[i] * a[i] + qr[i] * b[i] + qm[i] * a[i] * b[i] + qc[i]) * pow(qo[i], -1, R) % R
    cols = [ql, qr, qm, qo, qc, a, b, c]
    small, large = cfg.ntt_domain(pkg.NTT_ROOT_H2C, k), cfg.ntt_domain(pkg.NTT_ROOT_H2C, k + ext)
    try:
        w_big = m.decode(large.info()["omega"], g.MONT_LE)[0]
        w = pow(w_big, 1 << ext, R)
        assert m.decode(small.info()["omega"], g.MONT_LE)[0] == w
        shift = 7
        d_lag = dev.put(m.pack(cols, layout))
        cfg.ntt_device(small, d_lag, d_lag, pkg.NTT_INVERSE, layout, n_vec=8)
        coeff = m.tables(dev.get(d_lag, 32 * 8 * n), layout, n, 8)
        d_coeff = dev.put(m.pack([f + [0] * (big - n) for f in coeff], layout))
        d_coset, d_h = dev.put(b"\0" * 32 * 8 * big), dev.put(POISON * big)
        cfg.ntt_device(large, d_coeff, d_coset, pkg.NTT_FORWARD, layout, shift=m.encode([shift], layout), n_vec=8)
        zh_inv = [pow((pow(shift, n, R) * pow(w_big, n * i, R) - 1) % R, -1, R) for i in range(1 << ext)]
        gate = g.vanilla_next(1 << ext)
        _, ms = cfg.fr_gate_eval(d_coset, gate.lib_terms(pkg, layout), big, 8, rot_step=gate.rot_step, out=d_h,
                                 scale=m.encode(zh_inv, layout), scalar_layout=layout, mem=pkg.MEM_DEVICE)
        cfg.ntt_device(large, d_h, d_h, pkg.NTT_INVERSE, layout, shift=m.encode([shift], layout))
        h = m.decode(dev.get(d_h, 32 * big), layout)
        assert h[3 * (n - 1) - n + 1:] == [0] * (big - (3 * (n - 1) - n + 1)) and any(h), "the quotient is no polynomial of degree 13"
        x = rng.randrange(R)
        at_x, _ = cfg.fr_poly_eval_device(d_coeff, big, m.encode([x], layout), layout, n_vec=8)
        at_wx, _ = cfg.fr_poly_eval_device(d_coeff, big, m.encode([w * x], layout), layout, n_vec=8)
        h_x, _ = cfg.fr_poly_eval_device(d_h, big, m.encode([x], layout), layout)
        QL, QR, QM, QO, QC, A, B, _ = m.decode(at_x, layout)
        C_next = m.decode(at_wx, layout)[7]
        assert m.decode(h_x, layout)[0] * (pow(x, n, R) - 1) % R == (QL * A + QR * B + QM * A * B - QO * C_next + QC) % R
    finally:
        small.free()
        large.free()
