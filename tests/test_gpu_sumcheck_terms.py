"""The term-list sumcheck calls on the GPU (msm_amd_fr_sumcheck_round_terms, msm_amd_fr_sumcheck_step_terms; host and device memory) against the host
twins and the big-integer model of tests/terms_ref.py (tests/test_sumcheck_terms_host.py pins the twins to the model on the
CPU).  Every comparison is of bytes: device call = host-buffer call = twin = model.  MSM_AMD_FR_MLE_CHUNK_LOG = 6 brings every
geometry of the round plan -- one pair, one full wave, two waves and a fold, a fold over 128 partials, three levels -- down to
a few thousand records; the shapes are the smallest at which each path can go wrong."""
import ctypes
import random

import pytest

import mle_ref as m
import terms_ref as t
from guard import Arena, HostArena, In, Out, At, guarded

pytestmark = pytest.mark.gpu

R = m.R
POISON = b"\xFF" * 32
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Device:
    """device buffers of one test, freed together"""

    def __init__(self, cfg):
        self.cfg, self.ptrs = cfg, []

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
def dev(cfg):
    d = Device(cfg)
    yield d
    d.close()


def tables_of(form, seed, n, layout, stride, edge=False):
    if edge:
        return m.pack_raw(m.edge_tables(seed, n, form.n_vec), stride)
    return m.pack([m.random_values(seed + v, n) for v in range(form.n_vec)], layout, stride)


def device_round(dev, terms, data, layout, order, form, n, stride):
    d_in = dev.put(data)
    g, ms = dev.cfg.fr_sumcheck_round_terms_device(d_in, n, terms, order, layout, form.n_vec, stride)
    assert ms >= 0 and dev.get(d_in, len(data)) == data, "input changed"
    dev.close()
    return g


def device_step(dev, terms, data, r, layout, order, form, n, stride, in_place=False):
    """a step on fresh buffers: out of place into poison, and the input must survive; (all of the output buffer, g)"""
    size = 32 * (m.span(n, form.n_vec, stride) + 3)
    d_in = dev.put(data + POISON * 3 if in_place else data)
    d_out = d_in if in_place else dev.put(POISON * (size // 32))
    g, ms = dev.cfg.fr_sumcheck_step_terms_device(d_in, n, d_out, r, terms, order, layout, form.n_vec, stride)
    assert ms >= 0
    if not in_place:
        assert dev.get(d_in, len(data)) == data, "input changed"
    out = dev.get(d_out, size)
    dev.close()
    return out, g


def check_form(c, pkg, dev, form, mm, order, layout, seed, model=True, edge=False, strided=True):
    """round and step at n = 2^mm: device = host-buffer call = twin (= model); the step writes the first n / 2 records of every
    output table and nothing else, out of place and (HIGH) in place"""
    n = 1 << mm
    stride = n + 5 if strided else n
    tag = (form, mm, order, layout)
    terms = form.lib_terms(pkg, layout)
    data = tables_of(form, seed, n, layout, stride, edge)
    twin = pkg.host_fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec, stride, threads=16)
    if model:
        assert twin == t.round_values(data, layout, order, form, n, stride), tag
    assert len(twin) == 32 * (form.degree + 1)
    assert device_round(dev, terms, data, layout, order, form, n, stride) == twin, tag
    assert c.fr_sumcheck_round_terms(data, n, terms, order, layout, form.n_vec, stride) == twin, tag
    if mm < 2:
        return
    r = m.challenges(seed, 1, layout, edge=edge)
    poison = POISON * (m.span(n, form.n_vec, stride) + 3)
    t_out, t_g = pkg.host_fr_sumcheck_step_terms(data, r, n, terms, order, layout, form.n_vec, stride, threads=16, out=poison)
    t_tabs = m.bind_outputs(t_out, n, 1, form.n_vec, stride)
    if model:
        assert (t_tabs, t_g) == t.step(data, r, layout, order, form, n, stride), tag
    for in_place, before in [(False, poison)] + ([(True, data + POISON * 3)] if order == t.HIGH else []):
        out, g = device_step(dev, terms, data, r, layout, order, form, n, stride, in_place)
        assert g == t_g and m.bind_outputs(out, n, 1, form.n_vec, stride) == t_tabs, (tag, in_place)
        assert m.bind_untouched(out, before, n, form.n_vec, stride) is None, (tag, in_place)
    out, g = c.fr_sumcheck_step_terms(data, r, n, terms, order, layout, form.n_vec, stride, out=poison)
    assert g == t_g and m.bind_outputs(out, n, 1, form.n_vec, stride) == t_tabs, tag
    assert m.bind_untouched(out, poison, n, form.n_vec, stride) is None, tag


# ---- 1. geometry at MSM_AMD_FR_MLE_CHUNK_LOG = 6, every form ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx(msm_pkg):
    """MSM_AMD_FR_MLE_CHUNK_LOG is read at msm_amd_init"""
    mp = pytest.MonkeyPatch()
    mp.setenv("MSM_AMD_FR_MLE_CHUNK_LOG", "6")
    c2 = msm_pkg.setup_metal_state()
    mp.undo()
    yield c2
    c2.close()


@pytest.mark.parametrize("mm", [1, 2, 7, 8])
def test_small_geometry_every_form(msm_pkg, small_ctx, mm):
    """m = 1: one pair and 63 idle lanes; m = 2: one pair after the bind; m = 7: exactly one full wave; m = 8: two waves and a fold"""
    P = msm_pkg.test_fr_sumcheck_terms_plan
    terms = t.VANILLA.lib_terms(msm_pkg, m.MONT_LE)
    assert [P(terms, 1 << k, 9, 6)["first_waves"] for k in (1, 7, 8)] == [1, 1, 2] and P(terms, 1 << 8, 9, 6)["launches"] == 2
    dev = Device(small_ctx)
    try:
        for j, form in enumerate(t.FORMS):
            for order in t.ORDERS:
                layout = (mm + order + j) & 1
                check_form(small_ctx, msm_pkg, dev, form, mm, order, layout, 10 * mm + j, edge=(j + order) % 2 == 0, strided=j % 3 != 0)
    finally:
        dev.close()


@pytest.mark.parametrize("form", [t.VANILLA, t.FORMS[6], t.FORMS[3]], ids=repr)
def test_small_geometry_fold_over_128_partials(msm_pkg, small_ctx, form):
    assert msm_pkg.test_fr_sumcheck_terms_plan(form.lib_terms(msm_pkg, 0), 1 << 14, form.n_vec, 6)["first_waves"] == 128
    dev = Device(small_ctx)
    try:
        for order in t.ORDERS:
            check_form(small_ctx, msm_pkg, dev, form, 14, order, order, 14, model=False)
    finally:
        dev.close()


def test_small_geometry_three_levels(msm_pkg, small_ctx):
    form, mm, layout = t.GKR, 18, m.MONT_LE
    n = 1 << mm
    terms = form.lib_terms(msm_pkg, layout)
    assert msm_pkg.test_fr_sumcheck_terms_plan(terms, n, form.n_vec, 6)["launches"] == 3
    data = cached("three-levels", lambda: m.raw(random.Random(18).choices(m.random_values(18, 263), k=n * form.n_vec)))
    dev = Device(small_ctx)
    try:
        assert device_round(dev, terms, data, layout, t.HIGH, form, n, n) == \
            msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, t.HIGH, layout, form.n_vec, threads=16)
    finally:
        dev.close()


# ---- 2. the default knobs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mm", [1, 6, 9, 10, 16])
def test_default_knobs(cfg, msm_pkg, dev, mm):
    forms = (t.VANILLA, t.FORMS[6], t.FORMS[3], t.FORMS[2]) if mm < 16 else (t.VANILLA,)
    for j, form in enumerate(forms):
        for order in t.ORDERS:
            check_form(cfg, msm_pkg, dev, form, mm, order, (mm + order + j) & 1, mm + j, model=mm <= 6, edge=mm == 9)


# ---- 3. the shipped forms as term lists; the step as bind + round ---------------------------------------------------------------------
@pytest.mark.parametrize("mm", [1, 7, 10])
def test_lists_that_spell_the_shipped_forms(cfg, msm_pkg, dev, mm):
    """the bytes of msm_amd_fr_sumcheck_round_device on the same buffer: outputs are unique residues"""
    n = 1 << mm
    for layout in t.LAYOUTS:
        data = tables_of(t.EQ_AB_C, mm, n, layout, n + 4, edge=True)
        d_in = dev.put(data)
        for order in t.ORDERS:
            for form, shipped in [(t.product(k), m.PRODUCT) for k in (1, 2, 3, 4)] + [(t.EQ_AB_C, m.EQ_AB_C)]:
                got, _ = cfg.fr_sumcheck_round_terms_device(d_in, n, form.lib_terms(msm_pkg, layout), order, layout, form.n_vec, n + 4)
                assert got == cfg.fr_sumcheck_round_device(d_in, n, shipped, order, layout, form.n_vec, n + 4)[0], (layout, order, form)
        assert dev.get(d_in, len(data)) == data


@pytest.mark.parametrize("mm", [2, 8, 11])
def test_step_is_bind_then_round(cfg, msm_pkg, dev, mm):
    n = 1 << mm
    for j, form in enumerate((t.VANILLA, t.FORMS[6], t.FORMS[4])):
        for order in t.ORDERS:
            layout, stride = (j + order) & 1, n + 3 * j
            terms = form.lib_terms(msm_pkg, layout)
            data = tables_of(form, mm + j, n, layout, stride, edge=j == 2)
            r = m.challenges(mm, 1, layout)
            size = 32 * m.span(n, form.n_vec, stride)
            d_in, d_a, d_b = dev.put(data), dev.put(POISON * (size // 32)), dev.put(POISON * (size // 32))
            g_step, _ = cfg.fr_sumcheck_step_terms_device(d_in, n, d_a, r, terms, order, layout, form.n_vec, stride)
            cfg.fr_mle_bind_device(d_in, n, d_b, r, order, layout, form.n_vec, stride)
            g_pair, _ = cfg.fr_sumcheck_round_terms_device(d_b, n // 2, terms, order, layout, form.n_vec, stride)
            assert g_step == g_pair, (form, order)
            assert m.bind_outputs(dev.get(d_a, size), n, 1, form.n_vec, stride) == m.bind_outputs(dev.get(d_b, size), n, 1, form.n_vec, stride)
            dev.close()


# ---- 4. what the step writes, through the guard bands -----------------------------------------------------------------------------------
def step_writable(n, stride, n_vec):
    """include/msm_amd.h: "the first n / 2 records of every output table (at out + 32 v stride) are the bound table ... The call
    writes NO OTHER BYTE of out" """
    return [(32 * v * stride, 32 * (n // 2)) for v in range(n_vec)]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "stride_n_plus_3"])
@pytest.mark.parametrize("n", [4, 128, 256, 1024, 2048])
def test_step_writes_only_the_bound_halves(cfg, msm_pkg, n, strided):
    """the gaps between the tables and every upper half keep their fill; at the default chunk n = 1024 is one wave, 2048 two"""
    L, form = msm_pkg.lib(), t.FORMS[5]
    stride = n + 3 if strided else n
    fn, dev_mem = L.msm_amd_fr_sumcheck_step_terms, msm_pkg.MEM_DEVICE
    span = 32 * m.span(n, form.n_vec, stride)
    for order in t.ORDERS:
        layout = order
        terms = form.lib_terms(msm_pkg, layout)
        data = tables_of(form, n, n, layout, stride)
        r = m.challenges(n, 1, layout)
        t_out, exp_g = msm_pkg.host_fr_sumcheck_step_terms(data, r, n, terms, order, layout, form.n_vec, stride, out=bytes(span))
        exp_tabs = m.bind_outputs(t_out, n, 1, form.n_vec, stride)
        if n <= 256:
            assert (exp_tabs, exp_g) == t.step(data, r, layout, order, form, n, stride)
        places = [Out(span, writable=step_writable(n, stride, form.n_vec))]
        if order == t.HIGH:
            places.append(Out(data=data, writable=step_writable(n, stride, form.n_vec)))
        for out in places:
            g = ctypes.create_string_buffer(b"\xA5" * 288, 288)
            src = out if out.data is not None else In(data)
            with Arena(cfg) as arena:
                got, = guarded(arena, fn, cfg.h, dev_mem, layout, order, ctypes.addressof(terms.c), r, src, n, form.n_vec, stride, out, g, None)
            assert m.bind_outputs(got, n, 1, form.n_vec, stride) == exp_tabs, (order, out.data is not None)
            assert g.raw == exp_g + b"\xA5" * (288 - len(exp_g))                     # d + 1 records and not a byte more


def test_refused_steps_leave_everything_untouched(cfg, msm_pkg):
    L, form, n, layout = msm_pkg.lib(), t.FORMS[5], 64, m.MONT_LE
    fn, bad, dev_mem = L.msm_amd_fr_sumcheck_step_terms, msm_pkg.INPUT_ERROR, msm_pkg.MEM_DEVICE
    terms = form.lib_terms(msm_pkg, layout)
    tp = ctypes.addressof(terms.c)
    data = tables_of(form, 3, n, layout, n)
    r = m.challenges(3, 1, layout)
    g = ctypes.create_string_buffer(b"\xA5" * 256, 256)

    def refused(order, src, out):
        with Arena(cfg) as arena:
            guarded(arena, fn, cfg.h, dev_mem, layout, order, tp, r, src, n, form.n_vec, n, out, g, None, ok=bad)
        assert b"msm_amd_fr_sumcheck_step_terms:" in L.msm_amd_last_error(cfg.h)
        assert g.raw == b"\xA5" * 256

    io = Out(data=data)
    refused(t.LOW, io, io)                                   # LOW in place
    assert b"out of place only" in L.msm_amd_last_error(cfg.h)
    for order in t.ORDERS:
        io = Out(data=data + bytes(64))
        refused(order, io, At(io, 32))                       # a partial overlap, one record in
        assert b"disjoint" in L.msm_amd_last_error(cfg.h)
        io = Out(data=bytes(32 * n) + data)
        refused(order, At(io, 32 * n), io)                   # the output ends inside the input
        io = Out(data=data)
        refused(order, io, At(io, 8))                        # misaligned
        assert b"16-byte aligned" in L.msm_amd_last_error(cfg.h)


# ---- 5. the protocol: round_terms once, step_terms per challenge, the last variable by bind ----------------------------------------------
def vanilla_tables(n, seed, satisfied=True):
    """selector and witness tables of HyperPlonk's vanilla gate with q_L w_1 + q_R w_2 + q_M w_1 w_2 - q_O w_3 + q_C = 0 in every
    row; table 0 is left for eq"""
    rng = random.Random(seed)
    col = lambda: [rng.randrange(R) for _ in range(n)]                                                     # noqa: E731
    ql, qr, qm, qo, w1, w2, w3 = (col() for _ in range(7))
    qc = [-(ql[i] * w1[i] + qr[i] * w2[i] + qm[i] * w1[i] * w2[i] - qo[i] * w3[i]) % R for i in range(n)]
    if not satisfied:
        qc[n // 3] = (qc[n // 3] + 1) % R
    return [ql, qr, qm, qo, qc, w1, w2, w3]


@pytest.mark.parametrize("order", t.ORDERS, ids=["low", "high"])
def test_protocol_on_the_vanilla_gate(cfg, msm_pkg, dev, order):
    mm, layout, form = 10, m.MONT_LE, t.VANILLA
    n0 = 1 << mm
    coeffs = form.coeff_values(layout)
    terms = form.lib_terms(msm_pkg, layout)
    tau, rs = m.random_values(71, mm), m.random_values(72, mm)
    point = m.encode(rs, layout)
    rec = lambda s: point[32 * s:32 * s + 32]                                                              # noqa: E731
    cols = cached("vanilla", lambda: m.pack(vanilla_tables(n0, 70), layout))
    d_orig = dev.put(bytes(32 * n0) + cols)
    cfg.fr_eq_table_device(d_orig, m.encode(tau, layout), order, layout)
    data = dev.get(d_orig, 32 * 9 * n0)
    # HIGH binds in place; LOW goes between two buffers
    d_a, d_b = dev.put(data), dev.put(bytes(len(data)))
    n, claim = n0, 0                                                                                       # the gate holds in every row
    g, _ = cfg.fr_sumcheck_round_terms_device(d_a, n, terms, order, layout, 9, n0)
    for s in range(mm - 1):
        claim = m.verifier_step(claim, m.decode(g, layout), rs[s])
        d_to = d_a if order == t.HIGH else d_b
        g, _ = cfg.fr_sumcheck_step_terms_device(d_a, n, d_to, rec(s), terms, order, layout, 9, n0)
        d_a, d_b, n = d_to, d_a, n // 2
    claim = m.verifier_step(claim, m.decode(g, layout), rs[mm - 1])
    assert n == 2
    d_to = d_a if order == t.HIGH else d_b
    cfg.fr_mle_bind_device(d_a, 2, d_to, rec(mm - 1), order, layout, 9, n0)                               # the last variable
    finals = [m.decode(dev.get(d_to + 32 * v * n0, 32), layout)[0] for v in range(9)]
    assert claim == t.combine(form, coeffs, finals)
    assert m.encode(finals, layout) == cfg.fr_mle_eval_device(d_orig, n0, point, order, layout, 9)[0]
    assert dev.get(d_orig, len(data)) == data


def test_a_gate_that_does_not_hold_is_the_callers_finding(cfg, msm_pkg, dev):
    mm, layout, form = 10, m.MONT_LE, t.VANILLA
    n0 = 1 << mm
    terms = form.lib_terms(msm_pkg, layout)
    d_t = dev.put(bytes(32 * n0) + m.pack(vanilla_tables(n0, 70, satisfied=False), layout))
    cfg.fr_eq_table_device(d_t, m.encode(m.random_values(71, mm), layout), t.HIGH, layout)
    g = m.decode(cfg.fr_sumcheck_round_terms_device(d_t, n0, terms, t.HIGH, layout, 9)[0], layout)         # no error
    assert (g[0] + g[1]) % R != 0
    g = m.decode(cfg.fr_sumcheck_step_terms_device(d_t, n0, d_t, m.encode([5], layout), terms, t.HIGH, layout, 9)[0], layout)
    assert len(g) == 5


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------------
def test_stale_workspaces_change_nothing(cfg, msm_pkg, dev):
    mm, layout, form = 13, m.CANON_LE, t.VANILLA
    n = 1 << mm
    terms = form.lib_terms(msm_pkg, layout)
    data = tables_of(form, 9, n, layout, n)
    r = m.challenges(9, 1, layout)

    def run():
        return (device_round(dev, terms, data, layout, t.HIGH, form, n, n), device_round(dev, terms, data, layout, t.LOW, form, n, n),
                device_step(dev, terms, data, r, layout, t.LOW, form, n, n), device_step(dev, terms, data, r, layout, t.HIGH, form, n, n, True),
                cfg.fr_sumcheck_round_terms(data, n, terms, t.LOW, layout, 9), cfg.fr_sumcheck_step_terms(data, r, n, terms, t.HIGH, layout, 9))

    assert msm_pkg.test_fr_sumcheck_terms_plan(terms, n, 9, step=True)["launches"] == 2       # partial records in the workspace
    first = run()
    cfg.test_fill_workspaces(0xFF)
    assert run() == first
    cfg.test_fill_workspaces(0x00)
    assert run() == first
    assert first[0] == msm_pkg.host_fr_sumcheck_round_terms(data, n, terms, t.HIGH, layout, 9, threads=16)
    assert first[5][1] == msm_pkg.host_fr_sumcheck_step_terms(data, r, n, terms, t.HIGH, layout, 9, threads=16)[1]


def test_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    mm, layout, form = 7, m.MONT_LE, t.GKR
    n = 1 << mm
    terms = form.lib_terms(msm_pkg, layout)
    data = tables_of(form, 4, n, layout, n)
    r = m.challenges(4, 1, layout)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        d, d_o = c2.alloc(len(data)), c2.alloc(len(data))
        c2.to_device(d, data)
        c2.to_device(d_o, bytes(len(data)))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_sumcheck_round_terms", lambda: c2.fr_sumcheck_round_terms_device(d, n, terms, t.LOW, layout, 5)),
                           ("msm_amd_fr_sumcheck_round_terms", lambda: c2.fr_sumcheck_round_terms(data, n, terms, t.LOW, layout, 5)),
                           ("msm_amd_fr_sumcheck_step_terms", lambda: c2.fr_sumcheck_step_terms_device(d, n, d_o, r, terms, t.LOW, layout, 5)),
                           ("msm_amd_fr_sumcheck_step_terms", lambda: c2.fr_sumcheck_step_terms(data, r, n, terms, t.HIGH, layout, 5))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name + ":" in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data and c2.to_host(d_o, len(data)) == bytes(len(data))     # the refused calls wrote nothing
        assert c2.fr_sumcheck_round_terms_device(d, n, terms, t.LOW, layout, 5)[0] == t.round_values(data, layout, t.LOW, form, n)
        assert c2.fr_sumcheck_step_terms_device(d, n, d_o, r, terms, t.LOW, layout, 5)[0] == t.step(data, r, layout, t.LOW, form, n)[1]
        c2.free(d)
        c2.free(d_o)
    finally:
        c2.close()


def test_argument_errors_by_name_and_empty_calls(cfg, msm_pkg, dev):
    L, vp = msm_pkg.lib(), ctypes.c_void_p
    data = m.pack([m.random_values(v, 16) for v in range(2)], m.MONT_LE)
    one = m.encode([1], m.MONT_LE)
    d_in, d_out = dev.put(data), dev.put(b"\xA5" * len(data))
    g = ctypes.create_string_buffer(b"\xA5" * 256, 256)
    h, i_, o_ = cfg.h, vp(d_in), vp(d_out)
    ptr = lambda x: None if x is None else ctypes.addressof(x.c)                                          # noqa: E731
    RT, ST, HOST, DEV = L.msm_amd_fr_sumcheck_round_terms, L.msm_amd_fr_sumcheck_step_terms, msm_pkg.MEM_HOST, msm_pkg.MEM_DEVICE
    text = {"n_terms": b"n_terms must be 1 .. 16", "term": b"a term length must be 1 .. 6", "index": b"is not below n_vec",
            "outer": b"outer must be a table index", "n_vec": b"n_vec", "null": b"null", "layout": b"MSM_AMD_SCALAR_MONT_LE",
            "order": b"MSM_AMD_MLE_LOW", "n": b"power of two", "stride": b"stride < n"}
    for name, (terms, n, n_vec, stride, order, layout) in t.error_cases(msm_pkg).items():
        calls = (("msm_amd_fr_sumcheck_round_terms", lambda: RT(h, DEV, layout, order, ptr(terms), i_, n, n_vec, stride, g, None)),
                 ("msm_amd_fr_sumcheck_round_terms", lambda: RT(h, HOST, layout, order, ptr(terms), data, n, n_vec, stride, g, None)),
                 ("msm_amd_fr_sumcheck_step_terms", lambda: ST(h, DEV, layout, order, ptr(terms), one, i_, n, n_vec, stride, o_, g, None)),
                 ("msm_amd_fr_sumcheck_step_terms", lambda: ST(h, HOST, layout, order, ptr(terms), one, data, n, n_vec, stride, g, g, None)))
        for who, call in calls:
            assert call() == msm_pkg.INPUT_ERROR, (name, who)
            err = L.msm_amd_last_error(h)
            assert who.encode() + b":" in err and text[name.split()[0]] in err, (name, who, err)
    good = msm_pkg.SumcheckTerms([(one, [0, 1])])
    more = {"null in": lambda: RT(h, DEV, 0, 0, ptr(good), None, 16, 2, 16, g, None),
            "null g_out": lambda: RT(h, DEV, 0, 0, ptr(good), i_, 16, 2, 16, None, None),
            "misaligned in": lambda: RT(h, DEV, 0, 0, ptr(good), vp(d_in + 8), 16, 2, 16, g, None),
            "mem 2": lambda: RT(h, 2, 0, 0, ptr(good), i_, 16, 2, 16, g, None),
            "step: mem -1": lambda: ST(h, -1, 0, 1, ptr(good), one, i_, 16, 2, 16, o_, g, None),
            "step: n == 2": lambda: ST(h, DEV, 0, 1, ptr(good), one, i_, 2, 2, 2, o_, g, None),
            "step: null r": lambda: ST(h, DEV, 0, 1, ptr(good), None, i_, 16, 2, 16, o_, g, None),
            "step: null out": lambda: ST(h, DEV, 0, 1, ptr(good), one, i_, 16, 2, 16, None, g, None),
            "step: misaligned out": lambda: ST(h, DEV, 0, 1, ptr(good), one, i_, 16, 2, 16, vp(d_out + 4), g, None)}
    for name, call in more.items():
        assert call() == msm_pkg.INPUT_ERROR and b"_terms:" in L.msm_amd_last_error(h), name
        assert (b"mem must be" in L.msm_amd_last_error(h)) == ("mem" in name), name
    assert dev.get(d_out, len(data)) == b"\xA5" * len(data) and dev.get(d_in, len(data)) == data and g.raw == b"\xA5" * 256
    # nothing to do: OK, nothing touched, the list is not looked at
    assert RT(h, DEV, 0, 0, None, None, 3, 0, 0, None, None) == msm_pkg.OK
    assert ST(h, DEV, 0, 1, None, None, None, 0, 0, 0, None, None, None) == msm_pkg.OK
    assert RT(h, HOST, 0, 0, None, None, 0, 0, 0, None, None) == msm_pkg.OK
    assert ST(h, HOST, 0, 0, None, None, None, 0, 0, 0, None, None, None) == msm_pkg.OK
