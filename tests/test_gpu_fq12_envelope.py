"""The bound-limit corpus of tests/fq12_envelope.py on the device (test_fq12_op_kernel through msm_amd_test_fq12_ops: one
launch per op, one lane per record, raw limbs in and out): every record bit-exact with the host twin of the same source,
limbs included, and correct against the big-integer model.  The device build is where the bounds matter: the operands sit
in private memory or LDS and are walked with rolled loops, and the column sums are v_mad_u64_u32 chains."""
import ctypes

import pytest

import fq12_envelope as env
import guard
import pairing_ref as pr
from test_fq12_envelope_host import OP_IDS, bound_failures, model_failures, run_ops

pytestmark = pytest.mark.gpu


def device_and_twin(cfg, msm_pkg, op, recs):
    dev = run_ops(cfg.test_fq12_ops, op, recs)
    host = run_ops(msm_pkg.test_fq12_ops_host, op, recs)
    diff = [i for i, (d, h) in enumerate(zip(dev, host)) if d != h]
    print(f"\n{env.OP_NAMES[op]}: {len(recs)} records, device == host twin bit for bit: {len(recs) - len(diff)}")
    assert len(dev) == len(host) == len(recs)
    assert not diff, f"device and host twin differ in {len(diff)} records, first {[recs[i][0] for i in diff[:5]]}: " \
                     f"{dev[diff[0]]} vs {host[diff[0]]}"
    return dev


@pytest.mark.parametrize("op", OP_IDS, ids=[env.OP_NAMES[op] for op in OP_IDS])
def test_op_device(cfg, msm_pkg, op):
    recs = env.corpus(op)
    dev = device_and_twin(cfg, msm_pkg, op, recs)
    bad = model_failures(recs, dev)
    assert not bad, f"{len(bad)} of {len(recs)} differ from the model, first: {bad[:3]}"
    bad = bound_failures(op, recs, dev)
    assert not bad, f"{len(bad)} of {len(recs)} outside the contract, first: {bad[:3]}"


def test_cross_op_identities_device(cfg):
    recs = env.corpus(pr.FQ12_OP_SQR)
    a = env.flat(recs, 2)
    sq = env.split(cfg.test_fq12_ops(pr.FQ12_OP_SQR, a, a, len(recs)))
    mu = env.split(cfg.test_fq12_ops(pr.FQ12_OP_MUL, a, a, len(recs)))
    assert [pr.fq12_of(w) for w in sq] == [pr.fq12_of(w) for w in mu]
    cyc = [r for r in env.corpus(pr.FQ12_OP_CYCLO_SQR) if r[1] == "cyclo"]
    a = env.flat(cyc, 2)
    cs = env.split(cfg.test_fq12_ops(pr.FQ12_OP_CYCLO_SQR, a, a, len(cyc)))
    sq = env.split(cfg.test_fq12_ops(pr.FQ12_OP_SQR, a, a, len(cyc)))
    assert [pr.fq12_of(w) for w in cs] == [pr.fq12_of(w) for w in sq]


def test_batch_writes_its_records_and_nothing_else(cfg, msm_pkg):
    """a count that is no multiple of the 64 lanes of a workgroup, more than one workgroup: guard bands round the host
    buffers the call fills (tests/guard.py), and the records equal the twin's"""
    recs = env.corpus(pr.FQ12_OP_MUL)[:70]
    n = len(recs)
    assert n == 70
    as_bytes = lambda words: bytes((ctypes.c_uint32 * len(words))(*words))
    L = msm_pkg.lib()
    with guard.HostArena() as arena:
        out, = guard.guarded(arena, L.msm_amd_test_fq12_ops, cfg.h, pr.FQ12_OP_MUL, guard.In(as_bytes(env.flat(recs, 2))),
                             guard.In(as_bytes(env.flat(recs, 3))), guard.Out(432 * n), n)
    assert out == as_bytes(msm_pkg.test_fq12_ops_host(pr.FQ12_OP_MUL, env.flat(recs, 2), env.flat(recs, 3), n))
    with guard.HostArena() as arena:                         # a shorter count leaves the rest of the buffer alone
        out, = guard.guarded(arena, L.msm_amd_test_fq12_ops, cfg.h, pr.FQ12_OP_MUL, guard.In(as_bytes(env.flat(recs, 2))),
                             guard.In(as_bytes(env.flat(recs, 3))), guard.Out(432 * n, writable=[(0, 432 * 65)]), 65)
    assert cfg.test_fq12_op(pr.FQ12_OP_MUL, recs[64][2], recs[64][3]) == \
        list((ctypes.c_uint32 * 108).from_buffer_copy(out[432 * 64:432 * 65]))          # the one-record call forwards


def test_device_refuses_bad_arguments(cfg, msm_pkg):
    L = msm_pkg.lib()
    z = (ctypes.c_uint32 * 216)()
    out = (ctypes.c_uint32 * 216)(*([0xA5A5A5A5] * 216))
    for args in ((14, z, z, out, 2), (-1, z, z, out, 2), (pr.FQ12_OP_MUL, None, z, out, 2), (pr.FQ12_OP_MUL, z, None, out, 2),
                 (pr.FQ12_OP_MUL, z, z, None, 2), (pr.FQ12_OP_MUL, z, z, out, (1 << 20) + 1)):
        assert L.msm_amd_test_fq12_ops(cfg.h, *args) == msm_pkg.INPUT_ERROR, args[0]
        assert list(out) == [0xA5A5A5A5] * 216
    assert L.msm_amd_test_fq12_ops(cfg.h, pr.FQ12_OP_MUL, None, None, None, 0) == msm_pkg.OK
    assert L.msm_amd_test_fq12_ops(cfg.h, pr.FQ12_OP_MUL, z, z, out, 0) == msm_pkg.OK and list(out) == [0xA5A5A5A5] * 216
    assert L.msm_amd_test_fq12_op(cfg.h, 14, z, z, out) == msm_pkg.INPUT_ERROR
    assert L.msm_amd_test_fq12_op(cfg.h, pr.FQ12_OP_MUL, None, z, out) == msm_pkg.INPUT_ERROR
    with pytest.raises(ValueError):
        cfg.test_fq12_ops(pr.FQ12_OP_MUL, [0] * 107, [0] * 108, 1 + 1)
    assert cfg.test_fq12_ops(pr.FQ12_OP_MUL, [], [], 0) == []
