"""Host tests of the multilinear calls (no GPU): the twins msm_amd_host_fr_mle_bind, msm_amd_host_fr_mle_eval,
msm_amd_host_fr_eq_table and msm_amd_host_fr_sumcheck_round against the big-integer model of tests/mle_ref.py, byte for
byte; the identities that tie the four calls together; the sumcheck protocol run to its end with the model's verifier; every
argument error; the plan tap msm_amd_test_fr_mle_plan."""
import ctypes
import random

import pytest

import mle_ref as m

R = m.R
POISON = b"\xFF" * 32


def n_binds(mm):
    return sorted({k for k in (1, 2, 3, mm - 1, mm) if 1 <= k <= mm})


def check_bind(bind, data, r_all, layout, order, n, n_vec, stride, tag):
    """a bind call against the model at every n_bind of the list, into poisoned memory"""
    mm = n.bit_length() - 1
    for k in n_binds(mm):
        r = r_all[:32 * k]
        before = POISON * (m.span(n, n_vec, stride) + 3)
        out = bind(data, r, n, order, layout, n_vec, stride, out=before)
        assert m.bind_outputs(out, n, k, n_vec, stride) == m.bind(data, r, layout, order, n, n_vec, stride), (tag, k)
        assert m.bind_untouched(out, before, n, n_vec, stride) is None, (tag, k)


@pytest.mark.parametrize("mm", range(1, 11))
def test_twins_match_the_model(msm_pkg, mm):
    n = 1 << mm
    for order in m.ORDERS:
        for layout in m.LAYOUTS:
            tag = (mm, order, layout)
            point = m.challenges(mm, mm, layout)
            for n_vec, stride in ((1, n), (3, n), (3, n + 5)):
                data = m.pack([m.random_values(100 * mm + v, n) for v in range(n_vec)], layout, stride)
                check_bind(lambda *a, **kw: msm_pkg.host_fr_mle_bind(*a, threads=3, **kw), data, point, layout, order, n, n_vec,
                           stride, tag)
                assert msm_pkg.host_fr_mle_eval(data, point, n, order, layout, n_vec, stride) == \
                    m.evaluate(data, point, layout, order, n, n_vec, stride), tag
            assert m.first_difference(msm_pkg.host_fr_eq_table(point, order, layout), m.eq_table(point, layout, order)) is None, tag
            for form, k in m.SHAPES:
                for stride in (n, n + 5):
                    data = m.pack([m.random_values(7 * mm + v, n) for v in range(k)], layout, stride)
                    assert msm_pkg.host_fr_sumcheck_round(data, n, form, order, layout, k, stride) == \
                        m.round_values(data, layout, order, form, n, k, stride), (tag, form, k)


@pytest.mark.parametrize("mm", [1, 2, 5, 8])
def test_high_binds_in_place(msm_pkg, mm):
    n = 1 << mm
    L = msm_pkg.lib()
    for layout in m.LAYOUTS:
        for n_vec, stride in ((1, n), (3, n + 5)):
            data = m.pack([m.random_values(mm + v, n) for v in range(n_vec)], layout, stride)
            r = m.challenges(3, mm, layout)
            for k in n_binds(mm):
                buf = ctypes.create_string_buffer(data, len(data))
                assert L.msm_amd_host_fr_mle_bind(layout, m.HIGH, r, k, buf, n, n_vec, stride, 0, buf) == msm_pkg.OK
                assert m.bind_outputs(buf.raw, n, k, n_vec, stride) == m.bind(data, r[:32 * k], layout, m.HIGH, n, n_vec, stride)
                assert m.bind_untouched(buf.raw, data, n, n_vec, stride) is None


@pytest.mark.parametrize("mm", [1, 3, 6])
def test_edge_words_as_records_and_challenges(msm_pkg, mm):
    """0, 1, r - 1 and the raw words r, r + 1, 2^256 - 1: any 256-bit word is taken mod r, every output is reduced"""
    n = 1 << mm
    for order in m.ORDERS:
        for layout in m.LAYOUTS:
            point = m.challenges(5 + mm, mm, layout, edge=True)
            data = m.pack_raw(m.edge_tables(mm, n, 4))
            for word in m.EDGE_WORDS:
                flat = m.raw([word] * n)
                assert msm_pkg.host_fr_mle_eval(flat, point, n, order, layout) == m.evaluate(flat, point, layout, order, n)
                assert msm_pkg.host_fr_sumcheck_round(flat * 2, n, m.PRODUCT, order, layout, 2) == \
                    m.round_values(flat * 2, layout, order, m.PRODUCT, n, 2)
            check_bind(msm_pkg.host_fr_mle_bind, data, point, layout, order, n, 4, n, (mm, order, layout))
            assert msm_pkg.host_fr_mle_eval(data, point, n, order, layout, 4) == m.evaluate(data, point, layout, order, n, 4)
            assert msm_pkg.host_fr_eq_table(point, order, layout) == m.eq_table(point, layout, order)
            for form, k in m.SHAPES:
                assert msm_pkg.host_fr_sumcheck_round(data, n, form, order, layout, k) == \
                    m.round_values(data, layout, order, form, n, k), (mm, form, k)


def test_bytes_do_not_depend_on_the_thread_count(msm_pkg):
    n, layout = 1 << 13, m.MONT_LE                   # 2^12 pairs: four ranges of 2^10 at 16 threads
    data = m.pack([m.random_values(v, n) for v in range(4)], layout)
    point = m.challenges(1, 13, layout)
    for order in m.ORDERS:
        for threads in (16, 5):
            assert msm_pkg.host_fr_mle_bind(data, point[:64], n, order, layout, 4, threads=threads) == \
                msm_pkg.host_fr_mle_bind(data, point[:64], n, order, layout, 4, threads=1)
            assert msm_pkg.host_fr_mle_eval(data, point, n, order, layout, 4, threads=threads) == \
                msm_pkg.host_fr_mle_eval(data, point, n, order, layout, 4, threads=1)
            assert msm_pkg.host_fr_eq_table(point, order, layout, threads) == msm_pkg.host_fr_eq_table(point, order, layout, 1)
            for form, k in m.SHAPES:
                assert msm_pkg.host_fr_sumcheck_round(data, n, form, order, layout, k, threads=threads) == \
                    msm_pkg.host_fr_sumcheck_round(data, n, form, order, layout, k, threads=1)
    one = msm_pkg.host_fr_sumcheck_round(data, n, m.EQ_AB_C, m.HIGH, layout, 4, threads=1)
    assert one == m.round_values(data, layout, m.HIGH, m.EQ_AB_C, n, 4)


@pytest.mark.parametrize("mm", [1, 2, 5, 9])
def test_identities(msm_pkg, mm):
    n = 1 << mm
    for order in m.ORDERS:
        for layout in m.LAYOUTS:
            f = m.random_values(40 + mm, n)
            data = m.encode(f, layout)
            pv = m.random_values(50 + mm, mm)
            point, rev = m.encode(pv, layout), m.encode(pv[::-1], layout)
            y = msm_pkg.host_fr_mle_eval(data, point, n, order, layout)
            eq = msm_pkg.host_fr_eq_table(point, order, layout)
            # eval = sum eq f, through a PRODUCT round of two tables
            g = m.decode(msm_pkg.host_fr_sumcheck_round(eq + data, n, m.PRODUCT, order, layout, 2), layout)
            assert (g[0] + g[1]) % R == m.decode(y, layout)[0]
            # HIGH at p = LOW at the reversed p
            assert msm_pkg.host_fr_mle_eval(data, rev, n, 1 - order, layout) == y
            assert msm_pkg.host_fr_eq_table(rev, 1 - order, layout) == eq
            # sum eq = 1, through a PRODUCT round of one table
            g = m.decode(msm_pkg.host_fr_sumcheck_round(eq, n, m.PRODUCT, order, layout, 1), layout)
            assert (g[0] + g[1]) % R == 1
            # g(0) + g(1) = sum F over the whole tables
            for form, k in m.SHAPES:
                tabs = [m.random_values(60 + mm + v, n) for v in range(k)]
                g = m.decode(msm_pkg.host_fr_sumcheck_round(m.pack(tabs, layout), n, form, order, layout, k), layout)
                assert (g[0] + g[1]) % R == m.total(tabs, form), (mm, form, k)


@pytest.mark.parametrize("form,k", m.SHAPES)
def test_protocol_to_the_end(msm_pkg, form, k):
    """claim -> m rounds -> the final claim equals F of the evaluations"""
    mm = 8
    n0 = 1 << mm
    for order in m.ORDERS:
        layout = order
        tabs = [m.random_values(80 + v, n0) for v in range(k)]
        data = m.pack(tabs, layout)
        rs = m.random_values(90 + k, mm)
        claim, cur, n = m.total(tabs, form), data, n0
        for s in range(mm):
            g = m.decode(msm_pkg.host_fr_sumcheck_round(cur, n, form, order, layout, k, n0), layout)
            claim = m.verifier_step(claim, g, rs[s])
            cur = msm_pkg.host_fr_mle_bind(cur, m.encode([rs[s]], layout), n, order, layout, k, n0, out=cur)
            n //= 2
        finals = [m.decode(cur[32 * v * n0:32 * v * n0 + 32], layout)[0] for v in range(k)]
        assert claim == m.combine(form, finals)
        assert m.encode(finals, layout) == msm_pkg.host_fr_mle_eval(data, m.encode(rs, layout), n0, order, layout, k)
        model_rounds, model_tabs = m.prove(tabs, order, form, rs)
        assert [f[0] for f in model_tabs] == finals


def test_argument_errors(msm_pkg):
    L = msm_pkg.lib()
    n, be32 = 16, msm_pkg.SCALAR_CANON_BE32
    data = m.pack([m.random_values(v, n) for v in range(4)], m.MONT_LE)
    buf = ctypes.create_string_buffer(data, len(data) + 64)
    out = ctypes.create_string_buffer(len(data))
    r = m.challenges(1, 4, m.MONT_LE)
    g = ctypes.create_string_buffer(160)
    base = ctypes.addressof(buf)
    vp = ctypes.c_void_p
    bind, ev, eq, rnd = (L.msm_amd_host_fr_mle_bind, L.msm_amd_host_fr_mle_eval, L.msm_amd_host_fr_eq_table,
                         L.msm_amd_host_fr_sumcheck_round)
    bad = [
        bind(be32, 0, r, 1, buf, n, 1, n, 0, out), bind(7, 0, r, 1, buf, n, 1, n, 0, out),           # layout
        ev(be32, 0, r, buf, n, 1, n, 0, g), eq(be32, 0, r, 4, 0, out), rnd(be32, 0, 0, buf, n, 1, n, 0, g),
        bind(0, 2, r, 1, buf, n, 1, n, 0, out), ev(0, -1, r, buf, n, 1, n, 0, g),                     # order
        eq(0, 2, r, 4, 0, out), rnd(0, 5, 0, buf, n, 1, n, 0, g),
        rnd(0, 0, 2, buf, n, 1, n, 0, g), rnd(0, 0, -1, buf, n, 1, n, 0, g),                          # form
        rnd(0, 0, 0, buf, n, 5, n, 0, g), rnd(0, 0, 1, buf, n, 3, n, 0, g), rnd(0, 0, 1, buf, n, 1, n, 0, g),   # tables of a form
        bind(0, 0, r, 1, buf, 12, 1, 12, 0, out), bind(0, 0, r, 1, buf, 1, 1, 1, 0, out),             # n
        bind(0, 0, r, 1, buf, 0, 1, 0, 0, out), ev(0, 0, r, buf, 24, 1, 24, 0, g), rnd(0, 0, 0, buf, 1, 1, 1, 0, g),
        ev(0, 0, r, buf, 1 << 32, 1, 1 << 32, 0, g),
        bind(0, 0, r, 0, buf, n, 1, n, 0, out), bind(0, 0, r, 5, buf, n, 1, n, 0, out),               # n_bind
        bind(0, 0, r, 1, buf, n, 2, n - 1, 0, out), ev(0, 0, r, buf, n, 2, 8, 0, g),                  # stride < n
        rnd(0, 0, 0, buf, n, 2, n - 1, 0, g),
        bind(0, 0, r, 1, buf, n, 1 << 16, 1 << 16, 0, out), ev(0, 0, r, buf, n, 1 << 28, n, 0, g),    # n_vec stride >= 2^32
        rnd(0, 0, 0, buf, n, 2, 1 << 31, 0, g),
        bind(0, 0, None, 1, buf, n, 1, n, 0, out), bind(0, 0, r, 1, None, n, 1, n, 0, out),           # null pointers
        bind(0, 0, r, 1, buf, n, 1, n, 0, None), ev(0, 0, None, buf, n, 1, n, 0, g), ev(0, 0, r, None, n, 1, n, 0, g),
        ev(0, 0, r, buf, n, 1, n, 0, None), eq(0, 0, None, 4, 0, out), eq(0, 0, r, 4, 0, None),
        rnd(0, 0, 0, None, n, 1, n, 0, g), rnd(0, 0, 0, buf, n, 1, n, 0, None),
        eq(0, 0, r, 0, 0, out), eq(0, 0, r, 32, 0, out),                                              # m
        bind(0, 0, r, 1, buf, n, 1, n, 0, buf),                                                       # LOW in place
        bind(0, 0, r, 1, buf, n, 1, n, 0, vp(base + 32)), bind(0, 1, r, 1, buf, n, 1, n, 0, vp(base + 32)),     # partial overlap
        bind(0, 1, r, 1, vp(base + 32), n, 1, n, 0, buf), bind(0, 1, r, 1, buf, n, 4, n, 0, vp(base + 32 * n)),
        bind(0, 0, r, 1, vp(base + 32 * (n // 2 - 1)), n, 1, n, 0, buf),        # the last record of the output's n/2
    ]
    assert bad == [msm_pkg.INPUT_ERROR] * len(bad), [i for i, st in enumerate(bad) if st != msm_pkg.INPUT_ERROR]
    assert buf.raw[:len(data)] == data and out.raw == bytes(len(data))
    # nothing to do: OK, nothing touched -- whatever the other sizes say
    assert bind(0, 0, None, 0, None, 12, 0, 0, 0, None) == msm_pkg.OK and ev(0, 1, None, None, 0, 0, 0, 0, None) == msm_pkg.OK
    assert rnd(0, 0, 1, None, 3, 0, 0, 0, None) == msm_pkg.OK
    # right behind the input is disjoint from it; HIGH in place is allowed
    assert bind(0, 0, r, 1, buf, n, 2, n, 0, vp(base + 32 * 2 * n)) == msm_pkg.OK
    assert bind(0, 1, r, 1, buf, n, 2, n, 0, buf) == msm_pkg.OK


def test_plan_tap(msm_pkg):
    P = msm_pkg.test_fr_mle_plan
    B, E, Q, S = msm_pkg.MLE_CALL_BIND, msm_pkg.MLE_CALL_EVAL, msm_pkg.MLE_CALL_EQ_TABLE, msm_pkg.MLE_CALL_ROUND
    # a round: one wave up to 2^C pairs, then one wave per chunk and a fold of up to 2^10 partials per wave and value
    p = P(S, 1 << 7, 2, chunk_log=6)
    assert (p["launches"], p["levels"], p["first_waves"], p["values"], p["records"]) == (1, 1, 1, 3, 3)
    p = P(S, 1 << 8, 2, chunk_log=6)
    assert (p["launches"], p["first_waves"], p["records"], p["waves"]) == (2, 2, 3 * 2 + 3, 2 + 3)
    p = P(S, 1 << 14, 4, form=msm_pkg.SUMCHECK_EQ_AB_C, chunk_log=6)
    assert (p["launches"], p["first_waves"], p["values"], p["records"]) == (2, 128, 4, 4 * 128 + 4)
    p = P(S, 1 << 18, 1, chunk_log=6)
    assert (p["launches"], p["first_waves"], p["records"]) == (3, 1 << 11, 2 * ((1 << 11) + 2 + 1))
    p = P(S, 1 << 24, 4, chunk_log=10)
    assert (p["launches"], p["first_waves"], p["bytes"]) == (3, 1 << 13, 32 * 5 * ((1 << 13) + 8 + 1))
    assert P(S, 2, 3)["launches"] == 1 and P(S, 2, 3)["first_waves"] == 1
    # an evaluation: the levels of the scan plan, one launch each
    for n, tile_log in ((1 << 9, 9), (1 << 10, 9), (1 << 18, 9), (1 << 19, 9), (1 << 24, 9), (1 << 10, 2), (1 << 7, 3)):
        p, q = P(E, n, 3, tile_log=tile_log), msm_pkg.test_fr_plan(n, 3, tile_log)
        assert p["launches"] == p["levels"] == q["levels"] and p["records"] == q["records"] + 3 and p["first_waves"] == q["tiles"]
    assert P(E, 1 << 18, 1)["levels"] == 2 and P(E, 1 << 19, 1)["levels"] == 3 and P(E, 1 << 24, 1)["levels"] == 3
    assert P(E, 1 << 6, 1, tile_log=2)["levels"] == 3 and P(E, 1 << 10, 1, tile_log=2)["levels"] == 5
    # a bind: three variables per launch; LOW with more than one launch alternates through n_vec n / 8 records
    assert P(B, 1 << 10, 3, n_bind=3)["launches"] == 1 and P(B, 1 << 10, 3, n_bind=4)["launches"] == 2
    assert P(B, 1 << 10, 3, n_bind=10)["launches"] == 4
    assert P(B, 1 << 10, 3, n_bind=3)["records"] == 0 and P(B, 1 << 10, 3, n_bind=4)["records"] == 3 << 7
    assert P(B, 1 << 10, 3, order=msm_pkg.MLE_HIGH, n_bind=10)["records"] == 0
    assert P(B, 1 << 10, 3, n_bind=4)["values"] == 3 << 6
    # the eq table: one launch, eight outputs per lane from m = 9
    assert P(Q, 8)["waves"] == 4 and P(Q, 9)["waves"] == 1 and P(Q, 20)["waves"] == 1 << 11 and P(Q, 20)["values"] == 1 << 20
    for bad in (lambda: P(S, 1 << 8, 2, chunk_log=5), lambda: P(S, 1 << 8, 2, chunk_log=21), lambda: P(E, 1 << 8, 1, tile_log=10),
                lambda: P(S, 1 << 8, 5), lambda: P(S, 12, 1), lambda: P(B, 16, 1, n_bind=5), lambda: P(Q, 32), lambda: P(9, 16),
                lambda: P(S, 16, 0), lambda: P(S, 16, 1, order=2)):
        with pytest.raises(msm_pkg.MsmError):
            bad()
