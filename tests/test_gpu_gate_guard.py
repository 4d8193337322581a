"""Guard bands round the output of msm_amd_fr_gate_eval (tests/guard.py): the call writes the n records of `out` and no other
byte, in device memory and in host buffers, plain, accumulating and scaled; the columns -- the gaps of a strided input
included -- stay as they were; and a refused call (an overlap, nine offsets, a bad period) leaves `out` untouched.  The sizes
straddle the workgroup of 256 lanes, the unit one lane too many would write by."""
import pytest

import gate_ref as g
from guard import Arena, At, HostArena, In, Out, guarded

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1   # MSM_AMD_MEM_*


@pytest.fixture(scope="module")
def L(msm_pkg):
    return msm_pkg.lib()


def call(cfg, fn, mem, *args, ok=0):
    with Arena(cfg) as arena, HostArena() as host:
        return guarded(host if mem == HOST else arena, fn, cfg.h, mem, *args, ok=ok, host_arena=host)


@pytest.mark.parametrize("n", (1, 255, 257, 1000))
def test_the_call_writes_out_and_nothing_else(cfg, msm_pkg, L, n):
    gate, stride = g.NEIGHBOURS, n + 5
    for mem in (DEVICE, HOST):
        for layout in g.LAYOUTS:
            terms = gate.lib_terms(msm_pkg, layout)
            data = g.columns(n + mem, n, gate.n_vec, layout, stride)
            old, k_acc = g.records(1, n, layout), g.records(2, 1, layout)
            period = 8 if n % 8 == 0 else 1
            scale = g.records(3, period, layout)
            fn, tp = L.msm_amd_fr_gate_eval, msm_pkg._terms_ptr(terms)
            assert call(cfg, fn, mem, layout, 0, tp, In(data), n, gate.n_vec, stride, 1, None, None, 0, Out(32 * n), None) == \
                [g.evaluate(data, layout, gate, n, stride)]
            assert call(cfg, fn, mem, layout, g.ACCUMULATE, tp, In(data), n, gate.n_vec, stride, 1, k_acc, scale, period, Out(data=old),
                        None) == [g.evaluate(data, layout, gate, n, stride, old=old, k_acc=k_acc, scale=scale)]


def test_a_refused_call_leaves_out_untouched(cfg, msm_pkg, L):
    n, layout = 256, g.MONT_LE
    fn, bad = L.msm_amd_fr_gate_eval, msm_pkg.INPUT_ERROR
    good = g.NEIGHBOURS.lib_terms(msm_pkg, layout)
    nine = g.Gate("nine", 2, [(1, [(0, r) for r in range(5)]), (1, [(1, r) for r in range(5, 9)])]).lib_terms(msm_pkg, layout)
    data, scale = g.columns(3, n, 2, layout), g.records(3, 512, layout)
    for mem in (DEVICE, HOST):
        def refused(text, terms, src, dst, scale=None, period=0):
            call(cfg, fn, mem, layout, 0, msm_pkg._terms_ptr(terms), src, n, 2, n, 1, None, scale, period, dst, None, ok=bad)
            assert "msm_amd_fr_gate_eval: " + text in msm_pkg.lib().msm_amd_last_error(cfg.h).decode(), text

        refused("more than MSM_AMD_GATE_MAX_OFFSETS (8) distinct offsets", nine, In(data), Out(32 * n))
        for period in (0, 3, 512):
            refused("period must be a power of two, 1 .. 256, that divides n", good, In(data), Out(32 * n), scale, period)
        io = Out(data=data + b"\xFF" * 32 * n)   # out inside the columns: on the first record, on the last, in between
        for shift in (0, 32 * (2 * n - 1), 32 * n):
            refused("the output must be disjoint from all of the input", good, io, At(io, shift))
