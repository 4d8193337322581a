"""The 29-bit-limb field and point arithmetic (csrc/bn254_fq29.hip.h, bn254_ec29.hip.h) at the edges of its bounds
contract, on the host twin of the device code (msm_amd_test_op_raw_host: raw limbs in and out), against the big-integer
model oracle/fq29_ref.py: exact Montgomery values and limbs, the stated postconditions, the point invariant, and every
exceptional branch (doubling, vanish) at every filter multiple j the formulas can reach."""
import collections

import pytest

from oracle import fq29_ref as m

FIELD_OPS = [m.FE_MUL, m.FE_SQR, m.FE_MUL2, m.FE_SUB_K4E30, m.FE_SUB_K8E30, m.FE_SUB_K8E31, m.FE_SUB_K16E30,
             m.FE_SUB_K16E31, m.FE_NORM, m.FE_NEG, m.FE_NEG_WIDE, m.FE_CANONICAL, m.FE_TO_EXT, m.FE_PACK_UNPACK,
             m.FE_ZERO]
POINT_OPS = [m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ, m.PT_ADD, m.PT_DOUBLE]


def run_raw(run, op, corpus):
    a = [w for c in corpus for w in c[0]]
    b = [w for c in corpus for w in c[1]]
    out = run(op, a, b, len(corpus))
    return [out[m.RAW_OUT * i:m.RAW_OUT * i + m.RAW_OUT] for i in range(len(corpus))]


def field_failures(op, corpus, outs):
    return [(i, corpus[i][0][:18], bad) for i, r in enumerate(outs) if (bad := m.field_check(op, *corpus[i], r))]


def point_failures(op, corpus, outs):
    return [(i, c[3], bad) for i, (c, r) in enumerate(zip(corpus, outs)) if (bad := m.point_check(op, c[0], c[1], r,
                                                                                                     c[2], c[3]))]


@pytest.mark.parametrize("op", FIELD_OPS, ids=[m.OP_NAMES[op] for op in FIELD_OPS])
def test_field_op_at_the_bounds(msm_pkg, op):
    corpus = m.field_corpus(op)
    outs = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    bad = field_failures(op, corpus, outs)
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


@pytest.fixture(scope="module")
def point_corpora():
    return {op: m.point_corpus(op) for op in POINT_OPS}


@pytest.mark.parametrize("op", POINT_OPS, ids=[m.OP_NAMES[op] for op in POINT_OPS])
def test_point_op_at_the_invariant(msm_pkg, point_corpora, op):
    corpus = point_corpora[op]
    outs = run_raw(msm_pkg.test_op_raw_host, op, corpus)
    bad = point_failures(op, corpus, outs)
    assert not bad, f"{len(bad)} of {len(corpus)} wrong, first: {bad[:3]}"


def branch_table(point_corpora):
    counts = collections.Counter()
    for op in (m.PT_MADD, m.PT_MMADD, m.PT_ADD_NZ):
        for c in point_corpora[op]:
            counts[(op, *c[3])] += 1
    return counts


def test_branches_all_reached(point_corpora):
    """The coverage claim as a test: every (op, exceptional branch, filter multiple j) of oracle/fq29_ref.CLAIMED
    occurs in the point corpus."""
    counts = branch_table(point_corpora)
    print("\nreached (op, branch, j): " + ", ".join(f"{m.OP_NAMES[op]}/{br}/{j}={n}" for (op, br, j), n in
                                                  sorted(counts.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2] or 0))))
    missing = sorted(m.CLAIMED - set(counts), key=str)
    assert not missing, f"never reached: {missing}"


def test_bad_raw_arguments_refused(msm_pkg):
    rec = [0] * m.RAW_IN
    for op in (-1, 20, 99):
        with pytest.raises(msm_pkg.MsmError) as e:
            msm_pkg.test_op_raw_host(op, rec, rec, 1)
        assert e.value.status == msm_pkg.INPUT_ERROR
    with pytest.raises(ValueError):
        msm_pkg.test_op_raw_host(m.FE_MUL, rec[:-1], rec, 1)
