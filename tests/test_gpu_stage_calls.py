"""The six oldest blocking calls on the call driver of the vector calls (device_call.h): msm_amd_test_op, _raw, _g2,
msm_amd_prepare_buckets_indices, msm_amd_sort_buckets_indices, msm_amd_sort_pairs_device.  What they gained with it: a
ctx that is busy past its wait bound refuses them before anything is enqueued, by name; afterwards they compute what
their host twins (or the models of tests/test_gpu_stages.py) compute.  And the single-op kernels at counts around their
64-lane block, against the host twins."""
import random
import struct

import pytest

import g2_ref as g
import test_g2_host as th
from helpers import fq_be32
from oracle import bn254_ref as o
from oracle import fq29_ref as m

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def operands():
    """65 records per op family, as flat u32 lists per record: (a, b) of OP_FP_MUL, RAW_FE_MUL, G2_RAW_FQ2_MUL"""
    rng = random.Random(65)
    fp = [(fq_be32(rng.randrange(o.P)), fq_be32(rng.randrange(o.P))) for _ in range(65)]
    raw = [(list(a), list(b)) for a, b in m.field_corpus(m.FE_MUL)[:65]]
    fq2 = [(g.pad(x), g.pad(y)) for x, y in th.fq2_corpus(10, n=65)]
    assert len(raw) == 65 and len(fq2) == 65
    return {"fp": fp, "raw": raw, "fq2": fq2}


def _flat(recs, count):
    return [w for r in recs[:count] for w in r[0]], [w for r in recs[:count] for w in r[1]]


def _ops(cfg, msm_pkg):
    """family -> (device call, host twin, op)"""
    return {"fp": (cfg.test_op, msm_pkg.test_op_host, msm_pkg.OP_FP_MUL),
            "raw": (cfg.test_op_raw, msm_pkg.test_op_raw_host, msm_pkg.RAW_FE_MUL),
            "fq2": (cfg.test_op_g2, msm_pkg.test_op_g2_host, msm_pkg.G2_RAW_FQ2_MUL)}


@pytest.mark.parametrize("count", [1, 64, 65])
@pytest.mark.parametrize("family", ["fp", "raw", "fq2"])
def test_single_ops_around_one_block(cfg, msm_pkg, operands, family, count):
    dev, host, op = _ops(cfg, msm_pkg)[family]
    a, b = _flat(operands[family], count)
    assert dev(op, a, b, count) == host(op, a, b, count)


def test_calls_behind_a_held_stream_are_refused_by_name_and_recover(msm_pkg, operands):
    k = 0x1D2C3B4A5968778695A4B3C2D1E0F1E2D3C4B5A6978879605142332415061728 % o.R_ORDER
    pairs = [(7, 0), (3, 1)]
    pair_bytes = struct.pack("<4I", *[v for p in pairs for v in p])
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    ops = _ops(c2, msm_pkg)
    calls = [("msm_amd_test_op", lambda: ops["fp"][0](ops["fp"][2], *_flat(operands["fp"], 1), 1)),
             ("msm_amd_test_op_raw", lambda: ops["raw"][0](ops["raw"][2], *_flat(operands["raw"], 1), 1)),
             ("msm_amd_test_op_g2", lambda: ops["fq2"][0](ops["fq2"][2], *_flat(operands["fq2"], 1), 1)),
             ("msm_amd_prepare_buckets_indices", lambda: c2.prepare_buckets_indices(o.encode_scalar_be32(k), 1, 4, 1)),
             ("msm_amd_sort_buckets_indices", lambda: c2.sort_buckets_indices(pairs))]
    try:
        d = c2.alloc(len(pair_bytes))
        c2.to_device(d, pair_bytes)
        calls.append(("msm_amd_sort_pairs_device", lambda: c2.sort_pairs_device(d, 2)))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in calls:
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name + ":" in str(e.value), (name, e.value)
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(pair_bytes)) == pair_bytes        # the refused call wrote nothing
        got = [call() for _, call in calls]
        for fam, out in zip(("fp", "raw", "fq2"), got):
            _, host, op = ops[fam]
            assert out == host(op, *_flat(operands[fam], 1), 1), fam
        assert got[3] == o.prepare_buckets_indices([k], 4, 1)
        assert got[4] == sorted(pairs, key=lambda p: p[0])
        assert got[5] >= 0
        assert c2.to_host(d, len(pair_bytes)) == struct.pack("<4I", 3, 1, 7, 0)
        c2.free(d)
    finally:
        c2.close()
