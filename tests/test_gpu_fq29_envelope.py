"""The bound-limit corpus of tests/test_host_fq29_envelope.py on the device (test_op_raw_kernel: one launch per op,
raw limbs in and out): results bit-exact with the host twin of the same source, and correct against the big-integer
model oracle/fq29_ref.py.  The device build differs from the host one where bounds matter: limb32 register pins and
v_mad_u64_u32 column sums."""
import pytest

from oracle import fq29_ref as m
from test_host_fq29_envelope import FIELD_OPS, POINT_OPS, branch_table, field_failures, point_failures, run_raw

pytestmark = pytest.mark.gpu


def _device_vs_host(cfg, msm_pkg, op, corpus):
    dev = run_raw(cfg.test_op_raw, op, corpus)
    host = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    diff = [i for i, (d, h) in enumerate(zip(dev, host)) if d != h]
    print(f"\n{m.OP_NAMES[op]}: {len(corpus)} records, device == host bit-exact: {len(corpus) - len(diff)}")
    assert not diff, f"device and host twin differ in {len(diff)} records, first {diff[:5]}: {dev[diff[0]]} vs " \
                     f"{host[diff[0]]}"
    return dev


@pytest.mark.parametrize("op", FIELD_OPS, ids=[m.OP_NAMES[op] for op in FIELD_OPS])
def test_field_op_device(cfg, msm_pkg, op):
    corpus = m.field_corpus(op)
    dev = _device_vs_host(cfg, msm_pkg, op, corpus)
    bad = field_failures(op, corpus, dev)
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


@pytest.fixture(scope="module")
def point_corpora():
    return {op: m.point_corpus(op) for op in POINT_OPS}


@pytest.mark.parametrize("op", POINT_OPS, ids=[m.OP_NAMES[op] for op in POINT_OPS])
def test_point_op_device(cfg, msm_pkg, point_corpora, op):
    corpus = point_corpora[op]
    dev = _device_vs_host(cfg, msm_pkg, op, corpus)
    bad = point_failures(op, corpus, dev)
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


def test_device_branches_all_reached(point_corpora):
    counts = branch_table(point_corpora)
    print("\nreached on the device (op, branch, j): " + ", ".join(
        f"{m.OP_NAMES[op]}/{br}/{j}={n}" for (op, br, j), n in
        sorted(counts.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2] or 0))))
    assert not m.CLAIMED - set(counts)


def test_device_refuses_unknown_raw_op(cfg, msm_pkg):
    rec = [0] * m.RAW_IN
    with pytest.raises(msm_pkg.MsmError) as e:
        cfg.test_op_raw(20, rec, rec, 1)
    assert e.value.status == msm_pkg.INPUT_ERROR
