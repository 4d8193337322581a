"""The host side of the Poseidon calls (msm_amd_poseidon_constants, msm_amd_host_poseidon_*, msm_amd_test_poseidon_plan)
against the big-integer model of tests/poseidon_ref.py and the published circomlib answers.  No GPU."""
import ctypes

import pytest

import poseidon_ref as m

R = m.R
LAYOUTS = (m.MONT_LE, m.CANON_LE)
TS = (2, 3, 4, 5)
POISON = b"\xFF" * 32


def std(pkg, t, layout=m.MONT_LE):
    """(t, r_f, r_p, ark, mds) of the library's generator at circomlib's rounds"""
    return (t, m.R_F, m.R_P[t]) + pkg.poseidon_constants(t, scalar_layout=layout)


def model_permute(data, t, ark, mds, r_f, r_p, layout):
    vals = m.unpack(data, layout)
    out = []
    for k in range(0, len(vals), t):
        out += m.permute(vals[k:k + t], ark, mds, r_f, r_p)
    return m.pack(out, layout)


def model_hash(data, t, ark, mds, r_f, r_p, layout, tag=0):
    vals = m.unpack(data, layout)
    return m.pack([m.hash_one(vals[k:k + t - 1], ark, mds, r_f, r_p, tag) for k in range(0, len(vals), t - 1)], layout)


# ---- 1. constants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TS)
def test_generated_constants_equal_the_model(msm_pkg, t):
    ark, mds = m.constants(t)
    for layout in LAYOUTS:
        got_ark, got_mds = msm_pkg.poseidon_constants(t, m.R_F, m.R_P[t], layout)
        assert got_ark == m.pack(ark, layout) and got_mds == m.pack(mds, layout), (t, layout)


def test_first_words_are_circomlibs(msm_pkg):
    ark, mds = msm_pkg.poseidon_constants(3, scalar_layout=m.CANON_LE)
    assert int.from_bytes(ark[:32], "little") == 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e
    assert int.from_bytes(mds[:32], "little") == 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b
    ark2, _ = msm_pkg.poseidon_constants(2, scalar_layout=m.CANON_LE)
    assert int.from_bytes(ark2[:32], "little") == 0x09c46e9ec68e9bd4fe1faaba294cba38a71aa177534cdd1b6c7dc0dbd0abd7a7
    assert m.constants(3)[0][0] == int.from_bytes(ark[:32], "little") and m.constants(3)[1][0] == int.from_bytes(mds[:32], "little")


def test_other_rounds_give_other_constants(msm_pkg):
    for t, r_f, r_p in ((3, 2, 0), (2, 8, 1), (5, 4, 3), (4, 64, 64)):
        ark, mds = m.constants(t, r_f, r_p)
        assert msm_pkg.poseidon_constants(t, r_f, r_p, m.MONT_LE) == (m.pack(ark, m.MONT_LE), m.pack(mds, m.MONT_LE))
        assert len(set(ark)) == len(ark) and all(0 <= x < R for x in ark + mds)


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------
KNOWN = (([1], 18586133768512220936620570745912940619677854269274689475585506675881198879027),
         ([1, 2], 7853200120776062878684798364095072458815029376092732009249414926327459813530),
         ([1, 2, 3], 6542985608222806190361240322586112750744169038454362455181422643027100751666),
         ([1, 2, 3, 4], 18821383157269793795438455681495246036402687001665670618754263018637548127333),
         ([0, 0], 14744269619966411208579211824598458697587494354926760081771325075741142829156))
ROOT_0_TO_7 = 11780650233517635876913804110234352847867393797952240856403268682492028497284


@pytest.mark.parametrize("inputs,digest", KNOWN)
def test_known_answers(msm_pkg, inputs, digest):
    assert m.poseidon(inputs) == digest
    for layout in LAYOUTS:
        shape = std(msm_pkg, len(inputs) + 1, layout)
        assert msm_pkg.host_poseidon_hash(*shape, m.pack(inputs, layout), 1, layout) == m.enc(digest, layout)
        # the digest is word 0 of the permutation of [0, inputs]
        assert msm_pkg.host_poseidon_permute(*shape, m.pack([0] + inputs, layout), 1, layout)[:32] == m.enc(digest, layout)


def test_known_root(msm_pkg):
    for layout in LAYOUTS:
        tree, root = msm_pkg.host_poseidon_merkle_build(*std(msm_pkg, 3, layout), m.pack(range(8), layout), 8, layout)
        assert root == m.enc(ROOT_0_TO_7, layout) == tree[-32:] and len(tree) == 7 * 32


# ---- 3. twin = model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_permute_and_hash_equal_the_model(msm_pkg, t, layout):
    ark, mds = m.constants(t)
    shape = std(msm_pkg, t, layout)
    n = 5
    states = m.pack(m.random_values(t, n * t), layout)
    assert msm_pkg.host_poseidon_permute(*shape, states, n, layout) == model_permute(states, t, ark, mds, m.R_F, m.R_P[t], layout)
    groups = m.pack(m.random_values(10 + t, n * (t - 1)), layout)
    for tag in (None, 0, 7, R - 1):
        want = model_hash(groups, t, ark, mds, m.R_F, m.R_P[t], layout, tag or 0)
        assert msm_pkg.host_poseidon_hash(*shape, groups, n, layout, None if tag is None else m.enc(tag, layout)) == want, tag


@pytest.mark.parametrize("t,r_f,r_p", ((2, 8, 1), (3, 2, 0), (5, 2, 1), (4, 6, 0), (3, 64, 64)))
def test_callers_constants(msm_pkg, t, r_f, r_p):
    rounds = r_f + r_p
    ark, mds = m.random_values(1, rounds * t), m.random_values(2, t * t)
    for layout in LAYOUTS:
        c = (t, r_f, r_p, m.pack(ark, layout), m.pack(mds, layout))
        states = m.pack(m.random_values(3, 3 * t), layout)
        assert msm_pkg.host_poseidon_permute(*c, states, 3, layout) == model_permute(states, t, ark, mds, r_f, r_p, layout)
        groups = m.pack(m.random_values(4, 3 * (t - 1)), layout)
        assert msm_pkg.host_poseidon_hash(*c, groups, 3, layout, m.enc(5, layout)) == model_hash(groups, t, ark, mds, r_f, r_p, layout, 5)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_words_as_inputs_tag_and_constants(msm_pkg, layout):
    t, r_f, r_p = 3, 2, 1
    words = list(m.EDGE_WORDS)
    ark_w = (words * 3)[:(r_f + r_p) * t]
    mds_w = (words[::-1] * 3)[:t * t - 1] + [5]
    ark, mds = [m.dec(m.raw(w), layout) for w in ark_w], [m.dec(m.raw(w), layout) for w in mds_w]
    c = (t, r_f, r_p, b"".join(map(m.raw, ark_w)), b"".join(map(m.raw, mds_w)))
    states = b"".join(m.raw(w) for w in words + words[:2])           # two states of three records
    assert msm_pkg.host_poseidon_permute(*c, states, 2, layout) == model_permute(states, t, ark, mds, r_f, r_p, layout)
    groups = b"".join(m.raw(w) for w in words)                         # two groups of two records
    for tag_w in words:
        want = model_hash(groups, t, ark, mds, r_f, r_p, layout, m.dec(m.raw(tag_w), layout))
        assert msm_pkg.host_poseidon_hash(*c, groups, 2, layout, m.raw(tag_w)) == want
    # with the generated constants too: every output is the reduced residue
    shape = std(msm_pkg, 3, layout)
    A, M = m.constants(3)
    out = msm_pkg.host_poseidon_hash(*shape, groups, 2, layout, m.raw(words[3]))
    assert out == model_hash(groups, 3, A, M, m.R_F, m.R_P[3], layout, m.dec(m.raw(words[3]), layout))
    assert all(int.from_bytes(out[k:k + 32], "little") < R for k in (0, 32))


def test_thread_counts_change_no_byte(msm_pkg):
    t, layout, n = 4, m.CANON_LE, 83
    shape = std(msm_pkg, t, layout)
    states, groups = m.pack(m.random_values(5, n * t), layout), m.pack(m.random_values(6, n * (t - 1)), layout)
    leaves = m.pack(m.random_values(7, 81), layout)
    one = (msm_pkg.host_poseidon_permute(*shape, states, n, layout, threads=1),
           msm_pkg.host_poseidon_hash(*shape, groups, n, layout, threads=1),
           msm_pkg.host_poseidon_merkle_build(*shape, leaves, 81, layout, threads=1))
    A, M = m.constants(t)
    assert one[1] == model_hash(groups, t, A, M, m.R_F, m.R_P[t], layout)
    for threads in (3, 16, 0):
        assert one == (msm_pkg.host_poseidon_permute(*shape, states, n, layout, threads=threads),
                       msm_pkg.host_poseidon_hash(*shape, groups, n, layout, threads=threads),
                       msm_pkg.host_poseidon_merkle_build(*shape, leaves, 81, layout, threads=threads)), threads


def test_in_place_forms(msm_pkg):
    L = msm_pkg.lib()
    for t in TS:
        _, r_f, r_p, ark, mds = std(msm_pkg, t)
        n = 4
        states = m.pack(m.random_values(t, n * t), m.MONT_LE)
        buf = ctypes.create_string_buffer(states, len(states))
        assert L.msm_amd_host_poseidon_permute(t, r_f, r_p, 0, ark, mds, buf, n, 2, buf) == msm_pkg.OK
        assert buf.raw == msm_pkg.host_poseidon_permute(t, r_f, r_p, ark, mds, states, n)
    # a hash with t = 2: digest i replaces the record it came from
    _, r_f, r_p, ark, mds = std(msm_pkg, 2)
    data = m.pack(m.random_values(9, 6), m.MONT_LE)
    buf = ctypes.create_string_buffer(data, len(data))
    assert L.msm_amd_host_poseidon_hash(2, r_f, r_p, 0, ark, mds, None, buf, 6, 1, buf) == msm_pkg.OK
    assert buf.raw == msm_pkg.host_poseidon_hash(2, r_f, r_p, ark, mds, data, 6)


# ---- 4. trees and paths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,d", ((3, 1), (3, 4), (4, 3), (5, 2), (5, 1)))
def test_trees_and_paths(msm_pkg, t, d):
    a = t - 1
    n = a ** d
    A, M = m.constants(t)
    for layout in LAYOUTS:
        shape = std(msm_pkg, t, layout)
        values = m.random_values(20 + t + d, n)
        leaves = m.pack(values, layout)
        for tag in (0, 3):
            levels = m.tree(values, t, A, M, m.R_F, m.R_P[t], tag)
            tree, root = msm_pkg.host_poseidon_merkle_build(*shape, leaves, n, layout, m.enc(tag, layout) if tag else None)
            assert tree == m.pack(m.flat(levels), layout) and root == m.enc(levels[-1][0], layout), (t, d, layout, tag)
        idx = list(range(n)) + [n - 1, 0]
        paths = m.unpack(msm_pkg.host_poseidon_merkle_paths(t, leaves, n, tree, idx, layout, threads=3), layout)
        per = d * (a - 1)
        assert len(paths) == per * len(idx)
        for k, i in enumerate(idx):
            sib = paths[k * per:(k + 1) * per]
            assert sib == m.path(values, levels, a, i), (t, d, i)
            assert m.verify(values[i], i, sib, a, levels[-1][0], A, M, m.R_F, m.R_P[t], 3), (t, d, i)
        assert not m.verify(values[0] + 1, 0, paths[:per], a, levels[-1][0], A, M, m.R_F, m.R_P[t], 3)


def test_unreduced_leaves_are_taken_mod_r(msm_pkg):
    shape = std(msm_pkg, 3, m.CANON_LE)
    A, M = m.constants(3)
    leaves = b"".join(m.raw(w) for w in m.EDGE_WORDS)
    values = [w % R for w in m.EDGE_WORDS]
    levels = m.tree(values, 3, A, M, m.R_F, m.R_P[3])
    tree, root = msm_pkg.host_poseidon_merkle_build(*shape, leaves, 4, m.CANON_LE)
    assert tree == m.pack(m.flat(levels), m.CANON_LE) and root == tree[-32:]
    paths = msm_pkg.host_poseidon_merkle_paths(3, leaves, 4, tree, [2], m.CANON_LE)
    assert m.unpack(paths, m.CANON_LE) == m.path(values, levels, 2, 2)
    assert paths[:32] == m.enc(m.EDGE_WORDS[3], m.CANON_LE)          # the sibling leaf leaves as its reduced residue


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors(msm_pkg):
    L, be32 = msm_pkg.lib(), msm_pkg.SCALAR_CANON_BE32
    ark, mds = msm_pkg.poseidon_constants(3)
    a_out, m_out = ctypes.create_string_buffer(32 * 128 * 5), ctypes.create_string_buffer(32 * 25)
    data = ctypes.create_string_buffer(m.pack(m.random_values(1, 32), 0), 32 * 32)
    out = ctypes.create_string_buffer(32 * 32)
    idx = (ctypes.c_uint64 * 2)(0, 7)
    bad_idx = (ctypes.c_uint64 * 2)(0, 8)
    at = lambda buf, off: ctypes.c_void_p(ctypes.addressof(buf) + off)   # noqa: E731
    con = L.msm_amd_poseidon_constants
    per = lambda *a: L.msm_amd_host_poseidon_permute(*a)                  # noqa: E731
    hsh = lambda *a: L.msm_amd_host_poseidon_hash(*a)                     # noqa: E731
    bld = lambda *a: L.msm_amd_host_poseidon_merkle_build(*a)             # noqa: E731
    pth = lambda *a: L.msm_amd_host_poseidon_merkle_paths(*a)             # noqa: E731
    cases = {
        "constants: t below 2": lambda: con(1, 8, 56, 0, a_out, m_out),
        "constants: t above 5": lambda: con(6, 8, 56, 0, a_out, m_out),
        "constants: r_f odd": lambda: con(3, 7, 57, 0, a_out, m_out),
        "constants: r_f zero": lambda: con(3, 0, 57, 0, a_out, m_out),
        "constants: too many rounds": lambda: con(3, 8, 121, 0, a_out, m_out),
        "constants: null ark": lambda: con(3, 8, 57, 0, None, m_out),
        "constants: null mds": lambda: con(3, 8, 57, 0, a_out, None),
        "constants: BE32": lambda: con(3, 8, 57, be32, a_out, m_out),
        "constants: unknown layout": lambda: con(3, 8, 57, 9, a_out, m_out),
        "permute: t": lambda: per(6, 8, 57, 0, ark, mds, data, 1, 1, out),
        "permute: r_f odd": lambda: per(3, 3, 57, 0, ark, mds, data, 1, 1, out),
        "permute: rounds": lambda: per(3, 8, 122, 0, ark, mds, data, 1, 1, out),
        "permute: layout": lambda: per(3, 8, 57, be32, ark, mds, data, 1, 1, out),
        "permute: null ark": lambda: per(3, 8, 57, 0, None, mds, data, 1, 1, out),
        "permute: null mds": lambda: per(3, 8, 57, 0, ark, None, data, 1, 1, out),
        "permute: null in": lambda: per(3, 8, 57, 0, ark, mds, None, 1, 1, out),
        "permute: null out": lambda: per(3, 8, 57, 0, ark, mds, data, 1, 1, None),
        "permute: n >= 2^32": lambda: per(3, 8, 57, 0, ark, mds, data, 1 << 32, 1, out),
        "permute: partial overlap": lambda: per(3, 8, 57, 0, ark, mds, data, 2, 1, at(data, 32)),
        "hash: layout": lambda: hsh(3, 8, 57, 7, ark, mds, None, data, 1, 1, out),
        "hash: null in": lambda: hsh(3, 8, 57, 0, ark, mds, None, None, 1, 1, out),
        "hash: null out": lambda: hsh(3, 8, 57, 0, ark, mds, None, data, 1, 1, None),
        "hash: n >= 2^32": lambda: hsh(3, 8, 57, 0, ark, mds, None, data, 1 << 32, 1, out),
        "hash: t = 3 in place": lambda: hsh(3, 8, 57, 0, ark, mds, None, data, 4, 1, data),
        "hash: t = 3 digests inside the input": lambda: hsh(3, 8, 57, 0, ark, mds, None, data, 4, 1, at(data, 32 * 7)),
        "hash: t = 2 partial overlap": lambda: hsh(2, 8, 56, 0, ark, mds, None, data, 4, 1, at(data, 32)),
        "build: t = 2": lambda: bld(2, 8, 56, 0, ark, mds, None, data, 1, 1, out, None),
        "build: n_leaves = 0": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 0, 1, out, None),
        "build: n_leaves = 1": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 1, 1, out, None),
        "build: no power of 2": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 12, 1, out, None),
        "build: no power of 3": lambda: bld(4, 8, 56, 0, ark, mds, None, data, 8, 1, out, None),
        "build: n_leaves >= 2^32": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 1 << 32, 1, out, None),
        "build: layout": lambda: bld(3, 8, 57, be32, ark, mds, None, data, 8, 1, out, None),
        "build: null leaves": lambda: bld(3, 8, 57, 0, ark, mds, None, None, 8, 1, out, None),
        "build: null tree": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 8, 1, None, None),
        "build: tree over the leaves": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 8, 1, at(data, 32 * 7), None),
        "build: tree is the leaves": lambda: bld(3, 8, 57, 0, ark, mds, None, data, 8, 1, data, None),
        "paths: t = 2": lambda: pth(2, 0, data, 8, out, idx, 2, 1, out),
        "paths: t = 6": lambda: pth(6, 0, data, 8, out, idx, 2, 1, out),
        "paths: count": lambda: pth(3, 0, data, 12, at(data, 32 * 16), idx, 2, 1, out),
        "paths: layout": lambda: pth(3, be32, data, 8, at(data, 32 * 16), idx, 2, 1, out),
        "paths: index = n_leaves": lambda: pth(3, 0, data, 8, at(data, 32 * 16), bad_idx, 2, 1, out),
        "paths: null idx": lambda: pth(3, 0, data, 8, at(data, 32 * 16), None, 2, 1, out),
        "paths: null out": lambda: pth(3, 0, data, 8, at(data, 32 * 16), idx, 2, 1, None),
        "paths: null tree": lambda: pth(3, 0, data, 8, None, idx, 2, 1, out),
        "paths: out over the tree": lambda: pth(3, 0, data, 8, at(data, 32 * 16), idx, 2, 1, at(data, 32 * 20)),
        "paths: out over the leaves": lambda: pth(3, 0, data, 8, at(data, 32 * 16), idx, 2, 1, at(data, 32 * 4)),
        "paths: too many records": lambda: pth(3, 0, data, 8, at(data, 32 * 16), idx, 1 << 31, 1, out),
    }
    before = data.raw
    for name, case in cases.items():
        assert case() == msm_pkg.INPUT_ERROR, name
    assert data.raw == before and out.raw == bytes(32 * 32)
    # nothing to do: OK, nothing touched
    assert per(3, 8, 57, 0, ark, mds, None, 0, 1, None) == msm_pkg.OK
    assert hsh(3, 8, 57, 0, ark, mds, None, None, 0, 1, None) == msm_pkg.OK
    assert pth(3, 0, data, 8, at(data, 32 * 16), None, 0, 1, None) == msm_pkg.OK
    assert data.raw == before and out.raw == bytes(32 * 32)
    # digests right behind the input are disjoint from it
    assert hsh(3, 8, 57, 0, ark, mds, None, data, 4, 1, at(data, 32 * 8)) == msm_pkg.OK
    assert data.raw[32 * 8:32 * 12] == msm_pkg.host_poseidon_hash(3, 8, 57, ark, mds, before[:32 * 8], 4)


# ---- 6. the plan tap ----------------------------------------------------------------------------------------------------------
def test_plan_tap(msm_pkg):
    plan = msm_pkg.test_poseidon_plan
    assert plan(3, 64, 2) == {"launches": 4, "depth": 6, "nodes": 63, "tail_levels": 3, "tail_nodes": 7, "per_launch": [32, 16, 8, 7]}
    assert plan(4, 81, 2) == {"launches": 3, "depth": 4, "nodes": 40, "tail_levels": 2, "tail_nodes": 4, "per_launch": [27, 9, 4]}
    assert plan(5, 64, 2) == {"launches": 2, "depth": 3, "nodes": 21, "tail_levels": 2, "tail_nodes": 5, "per_launch": [16, 5]}
    assert plan(3, 2, 2) == {"launches": 1, "depth": 1, "nodes": 1, "tail_levels": 1, "tail_nodes": 1, "per_launch": [1]}
    assert plan(3, 64, 0)["per_launch"] == [32, 16, 8, 4, 2, 1] and plan(3, 64, 0)["tail_levels"] == 1
    assert plan(3, 64, 10) == {"launches": 1, "depth": 6, "nodes": 63, "tail_levels": 6, "tail_nodes": 63, "per_launch": [63]}
    big = plan(3, 1 << 20, 8)
    assert big["launches"] == 12 and big["tail_levels"] == 9 and big["nodes"] == (1 << 20) - 1 and big["per_launch"][-1] == 511
    for t, n in ((3, 1 << 12), (4, 3 ** 7), (5, 4 ** 6)):
        for top in range(11):
            p = plan(t, n, top)
            assert sum(p["per_launch"]) == p["nodes"] == (n - 1) // (t - 2)
            assert p["launches"] - 1 + p["tail_levels"] == p["depth"]
            assert all(c > 1 << top for c in p["per_launch"][:-1])
    for bad in ((2, 4, 2), (6, 4, 2), (3, 12, 2), (3, 1, 2), (3, 0, 2), (3, 64, 11), (3, 1 << 32, 2)):
        with pytest.raises(msm_pkg.MsmError):
            plan(*bad)
