"""The Poseidon calls on the GPU (msm_amd_poseidon_permute*, _hash*, _merkle_build*, _merkle_paths*) against the host twins
and the big-integer model of tests/poseidon_ref.py (tests/test_poseidon_host.py pins the twins to the model on the CPU).
Every comparison is of bytes: device call = host-buffer call = twin = model.  MSM_AMD_POSEIDON_TOP_LOG = 2 brings the
level launches and the one-workgroup tail of a tree down to a few dozen leaves."""
import ctypes

import pytest

import poseidon_ref as m

pytestmark = pytest.mark.gpu

R = m.R
TS = (2, 3, 4, 5)
LAYOUTS = (m.MONT_LE, m.CANON_LE)
NS = (1, 63, 64, 65, 257)            # a lane tail, a full wave, one lane more, more than one workgroup
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


def shape(pkg, t, layout=m.MONT_LE):
    return (t, m.R_F, m.R_P[t]) + cached(("constants", t, layout), lambda: pkg.poseidon_constants(t, scalar_layout=layout))


def build_params(c, pkg):
    return {t: c.poseidon_params_build(*shape(pkg, t)) for t in TS}


@pytest.fixture(scope="module")
def params(cfg, msm_pkg):
    """the circomlib instances t = 2 .. 5 on the session's ctx"""
    p = build_params(cfg, msm_pkg)
    yield p
    for h in p.values():
        h.free()


@pytest.fixture(scope="module")
def small(msm_pkg):
    """a ctx whose trees keep only levels of at most four nodes for the last workgroup, and its instances"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSM_AMD_POSEIDON_TOP_LOG", "2")       # read at msm_amd_init
        c2 = msm_pkg.setup_metal_state()
    p = build_params(c2, msm_pkg)
    yield c2, p
    c2.close()                                           # msm_amd_destroy frees the handles left


def model_states(t):
    """257 random states and their permutations, as integers"""
    def make():
        A, M = m.constants(t)
        vals = m.random_values(100 + t, NS[-1] * t)
        out = []
        for k in range(0, len(vals), t):
            out += m.permute(vals[k:k + t], A, M, m.R_F, m.R_P[t])
        return vals, out
    return cached(("states", t), make)


def model_digests(t, tag):
    def make():
        A, M = m.constants(t)
        vals = m.random_values(200 + t, NS[-1] * (t - 1))
        return vals, [m.hash_one(vals[k:k + t - 1], A, M, m.R_F, m.R_P[t], tag) for k in range(0, len(vals), t - 1)]
    return cached(("digests", t, tag), make)


# ---- 1. permutations and hashes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TS)
def test_permute(cfg, msm_pkg, dev, params, t):
    vals, want = model_states(t)
    for layout in LAYOUTS:
        for n in NS:
            data, exp = m.pack(vals[:n * t], layout), m.pack(want[:n * t], layout)
            assert msm_pkg.host_poseidon_permute(*shape(msm_pkg, t), m.pack(vals[:n * t], m.MONT_LE), n) == m.pack(want[:n * t], m.MONT_LE)
            assert cfg.poseidon_permute(params[t], data, n, layout) == exp, (t, layout, n)
            d_in, d_out = dev.put(data + POISON), dev.put(POISON * (n * t + 1))
            assert cfg.poseidon_permute_device(params[t], d_in, n, d_out, layout) >= 0
            assert dev.get(d_out, len(exp) + 32) == exp + POISON, (t, layout, n)
            assert dev.get(d_in, len(data) + 32) == data + POISON, "input changed"
            assert cfg.poseidon_permute_device(params[t], d_in, n, d_in, layout) >= 0             # in place
            assert dev.get(d_in, len(exp) + 32) == exp + POISON, (t, layout, n)
            dev.close()


@pytest.mark.parametrize("t", TS)
def test_hash(cfg, msm_pkg, dev, params, t):
    for layout in LAYOUTS:
        tag = 0 if layout == m.MONT_LE else R - 2
        tag32 = m.enc(tag, layout) if tag else None
        vals, want = model_digests(t, tag)
        for n in NS:
            data, exp = m.pack(vals[:n * (t - 1)], layout), m.pack(want[:n], layout)
            assert msm_pkg.host_poseidon_hash(*shape(msm_pkg, t, layout), data, n, layout, tag32) == exp, (t, layout, n)
            assert cfg.poseidon_hash(params[t], data, n, layout, tag32) == exp, (t, layout, n)
            d_in, d_out = dev.put(data + POISON), dev.put(POISON * (n + 1))
            assert cfg.poseidon_hash_device(params[t], d_in, n, d_out, layout, tag32) >= 0
            assert dev.get(d_out, len(exp) + 32) == exp + POISON, (t, layout, n)
            assert dev.get(d_in, len(data) + 32) == data + POISON, "input changed"
            if t == 2:                                                                          # digest i over record i
                assert cfg.poseidon_hash_device(params[t], d_in, n, d_in, layout, tag32) >= 0
                assert dev.get(d_in, len(exp) + 32) == exp + POISON, (layout, n)
            dev.close()


def test_edge_words(cfg, msm_pkg, dev, params):
    words = list(m.EDGE_WORDS)
    for layout in LAYOUTS:
        groups = b"".join(m.raw(w) for w in words)
        for tag_w in words:
            twin = msm_pkg.host_poseidon_hash(*shape(msm_pkg, 3, layout), groups, 2, layout, m.raw(tag_w))
            d_in, d_out = dev.put(groups), dev.put(POISON * 2)
            assert cfg.poseidon_hash_device(params[3], d_in, 2, d_out, layout, m.raw(tag_w)) >= 0
            assert dev.get(d_out, 64) == twin == cfg.poseidon_hash(params[3], groups, 2, layout, m.raw(tag_w))
            dev.close()
        states = b"".join(m.raw(w) for w in words + words)
        assert cfg.poseidon_permute(params[4], states, 2, layout) == msm_pkg.host_poseidon_permute(*shape(msm_pkg, 4, layout), states, 2, layout)


def test_known_answers_through_the_device(cfg, msm_pkg, dev, params):
    known = (([1], 18586133768512220936620570745912940619677854269274689475585506675881198879027),
             ([1, 2], 7853200120776062878684798364095072458815029376092732009249414926327459813530),
             ([1, 2, 3], 6542985608222806190361240322586112750744169038454362455181422643027100751666),
             ([1, 2, 3, 4], 18821383157269793795438455681495246036402687001665670618754263018637548127333),
             ([0, 0], 14744269619966411208579211824598458697587494354926760081771325075741142829156))
    for inputs, digest in known:
        t = len(inputs) + 1
        for layout in LAYOUTS:
            d_in, d_out = dev.put(m.pack(inputs, layout)), dev.put(POISON)
            assert cfg.poseidon_hash_device(params[t], d_in, 1, d_out, layout) >= 0
            assert dev.get(d_out, 32) == m.enc(digest, layout) == cfg.poseidon_hash(params[t], m.pack(inputs, layout), 1, layout)
            dev.close()
    d_leaves, d_tree = dev.put(m.pack(range(8), m.CANON_LE)), dev.put(POISON * 7)
    root, ms = cfg.poseidon_merkle_build_device(params[3], d_leaves, 8, d_tree, m.CANON_LE)
    assert ms >= 0 and root == m.enc(11780650233517635876913804110234352847867393797952240856403268682492028497284, m.CANON_LE)


def test_callers_constants(cfg, msm_pkg, dev):
    for t, r_f, r_p in ((2, 8, 1), (3, 2, 0), (5, 64, 64)):
        ark, mds = m.random_values(1, (r_f + r_p) * t), m.random_values(2, t * t)
        h = cfg.poseidon_params_build(t, r_f, r_p, m.pack(ark, m.CANON_LE), m.pack(mds, m.CANON_LE), m.CANON_LE)
        assert h.info() == {"t": t, "r_f": r_f, "r_p": r_p, "device_bytes": 32 * ((r_f + r_p + 1) * t + t * t)}
        vals = m.random_values(3, 70 * t)
        want = []
        for k in range(0, len(vals), t):
            want += m.permute(vals[k:k + t], ark, mds, r_f, r_p)
        assert cfg.poseidon_permute(h, m.pack(vals, m.MONT_LE), 70) == m.pack(want, m.MONT_LE)
        h.free()


# ---- 2. trees and paths -------------------------------------------------------------------------------------------------------
def check_tree(c, pkg, p, t, d, layout, tag, seed):
    """device = host-buffer call = twin = model for the tree and for the paths of the first, the last and middle leaves"""
    a = t - 1
    n = a ** d
    A, M = m.constants(t)
    values = cached(("leaves", seed, n), lambda: m.random_values(seed, n))
    levels = cached(("levels", seed, t, n, tag), lambda: m.tree(values, t, A, M, m.R_F, m.R_P[t], tag))
    nodes = (n - 1) // (a - 1)
    leaves, exp = m.pack(values, layout), m.pack(m.flat(levels), layout)
    tag32 = m.enc(tag, layout) if tag else None
    assert len(exp) == 32 * nodes
    assert pkg.host_poseidon_merkle_build(*shape(pkg, t, layout), leaves, n, layout, tag32) == (exp, exp[-32:])
    assert c.poseidon_merkle_build(p[t], leaves, n, layout, tag32) == (exp, exp[-32:]), (t, d, layout)
    dv = Device(c)
    try:
        d_leaves, d_tree = dv.put(leaves + POISON), dv.put(POISON * (nodes + 1))
        root, ms = c.poseidon_merkle_build_device(p[t], d_leaves, n, d_tree, layout, tag32)
        assert ms >= 0 and root == exp[-32:], (t, d, layout)
        assert dv.get(d_tree, len(exp) + 32) == exp + POISON, (t, d, layout)
        assert dv.get(d_leaves, len(leaves) + 32) == leaves + POISON, "leaves changed"
        assert c.poseidon_merkle_build_device(p[t], d_leaves, n, d_tree, layout, tag32, want_root=False)[0] is None
        idx = sorted({0, n - 1, n // 2, n // 3, min(n - 1, 65)}) + [n - 1]
        per = d * (a - 1)
        want = m.pack(sum((m.path(values, levels, a, i) for i in idx), []), layout)
        assert pkg.host_poseidon_merkle_paths(t, leaves, n, exp, idx, layout) == want
        assert c.poseidon_merkle_paths(p[t], leaves, n, exp, idx, layout) == want, (t, d, layout)
        d_out = dv.put(POISON * (per * len(idx) + 1))
        assert c.poseidon_merkle_paths_device(p[t], d_leaves, n, d_tree, idx, d_out, layout) >= 0
        assert dv.get(d_out, len(want) + 32) == want + POISON, (t, d, layout)
        for k, i in enumerate(idx):
            assert m.verify(values[i], i, m.unpack(want[32 * per * k:32 * per * (k + 1)], layout), a, levels[-1][0], A, M, m.R_F,
                            m.R_P[t], tag)
    finally:
        dv.close()


@pytest.mark.parametrize("t,d", ((3, 6), (4, 4), (5, 3), (3, 1), (5, 1), (3, 2)))
def test_trees_at_top_log_2(msm_pkg, small, t, d):
    c2, p = small
    plan = msm_pkg.test_poseidon_plan(t, (t - 1) ** d, 2)
    if (t, d) == (3, 6):
        assert plan["per_launch"] == [32, 16, 8, 7]              # three level launches, then the one-workgroup tail
    if (t, d) == (4, 4):
        assert plan["per_launch"] == [27, 9, 4]                  # levels 27 / 9 / 3 / 1: none a multiple of 64
    if d == 1:
        assert plan["launches"] == 1
    for layout in LAYOUTS:
        check_tree(c2, msm_pkg, p, t, d, layout, 0 if layout else 9, 300 + t)


@pytest.mark.parametrize("t,d", ((3, 8), (3, 9), (3, 12), (4, 6), (5, 5)))
def test_trees_at_the_default_knobs(cfg, msm_pkg, params, t, d):
    """2^8: all in the last workgroup; 2^9: its first level has 2^TOP nodes; beyond: level launches in front of it"""
    assert msm_pkg.test_poseidon_plan(3, 1 << 9, 8)["launches"] == 1 and msm_pkg.test_poseidon_plan(3, 1 << 12, 8)["launches"] == 4
    check_tree(cfg, msm_pkg, params, t, d, (t + d) & 1, 0, 400 + t)


# ---- 3. the driver -------------------------------------------------------------------------------------------------------------
def test_stale_workspaces_change_nothing(cfg, msm_pkg, params):
    layout = m.CANON_LE
    states, groups = m.pack(m.random_values(1, 70 * 4), layout), m.pack(m.random_values(2, 70 * 2), layout)
    leaves = m.pack(m.random_values(3, 1 << 10), layout)

    def run():
        tree, root = cfg.poseidon_merkle_build(params[3], leaves, 1 << 10, layout)
        return (cfg.poseidon_permute(params[4], states, 70, layout), cfg.poseidon_hash(params[3], groups, 70, layout), tree, root,
                cfg.poseidon_merkle_paths(params[3], leaves, 1 << 10, tree, [0, 517, 1023], layout))

    first = run()
    cfg.test_fill_workspaces(0xFF)
    assert run() == first
    cfg.test_fill_workspaces(0x00)
    assert run() == first
    assert first[1] == msm_pkg.host_poseidon_hash(*shape(msm_pkg, 3, layout), groups, 70, layout)
    assert first[2:4] == msm_pkg.host_poseidon_merkle_build(*shape(msm_pkg, 3, layout), leaves, 1 << 10, layout)


def test_handle_misuse(cfg, msm_pkg, dev, params, small):
    c2, p2 = small
    data = m.pack(m.random_values(5, 8), m.MONT_LE)
    d_in, d_out = dev.put(data), dev.put(b"\xA5" * 512)
    idx = [0]

    def calls(c, h):
        return (("msm_amd_poseidon_permute_device", lambda: c.poseidon_permute_device(h, d_in, 2, d_out)),
                ("msm_amd_poseidon_hash_device", lambda: c.poseidon_hash_device(h, d_in, 2, d_out)),
                ("msm_amd_poseidon_merkle_build_device", lambda: c.poseidon_merkle_build_device(h, d_in, 4, d_out)),
                ("msm_amd_poseidon_merkle_paths_device", lambda: c.poseidon_merkle_paths_device(h, d_in, 4, d_out, idx, d_out + 256)),
                ("msm_amd_poseidon_permute", lambda: c.poseidon_permute(h, data, 2)),
                ("msm_amd_poseidon_hash", lambda: c.poseidon_hash(h, data, 2)),
                ("msm_amd_poseidon_merkle_build", lambda: c.poseidon_merkle_build(h, data, 4)),
                ("msm_amd_poseidon_merkle_paths", lambda: c.poseidon_merkle_paths(h, data, 4, data[:96], idx)),
                ("msm_amd_poseidon_params_info", lambda: msm_pkg.PoseidonParams(c, h).info()),
                ("msm_amd_poseidon_params_free", lambda: msm_pkg.PoseidonParams(c, h).free()))

    freed = cfg.poseidon_params_build(*shape(msm_pkg, 3))
    freed.free()
    mat = cfg.fr_matrix_build(1, 1, [0, 0], None, None)
    try:
        for what, h in (("freed", freed.h), ("a matrix", mat.h), ("of another ctx", p2[3].h), ("null", ctypes.c_void_p())):
            for name, call in calls(cfg, h):
                with pytest.raises(msm_pkg.MsmError) as e:
                    call()
                assert e.value.status == msm_pkg.INPUT_ERROR and name in str(e.value), (what, name, e.value)
        for name, call in calls(c2, params[3].h)[:2]:                # and the session's handle on the other ctx
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.INPUT_ERROR and name in str(e.value), e.value
        with pytest.raises(msm_pkg.MsmError):                       # a Poseidon handle is no matrix
            cfg.fr_matvec_device(params[3].h, d_in, d_out)
        assert dev.get(d_out, 512) == b"\xA5" * 512 and dev.get(d_in, len(data)) == data
        assert params[3].info()["t"] == 3 and p2[3].info()["r_p"] == 57       # the live handles are untouched
    finally:
        mat.free()


def test_calls_behind_a_held_stream_time_out_and_recover(msm_pkg):
    layout = m.MONT_LE
    values = m.random_values(6, 16)
    data = m.pack(values, layout)
    c2 = msm_pkg.setup_metal_state()          # a fresh ctx: no buffer of these calls is sized yet
    try:
        h = c2.poseidon_params_build(*shape(msm_pkg, 3))
        d, d_o = c2.alloc(len(data)), c2.alloc(1024)
        c2.to_device(d, data)
        c2.to_device(d_o, bytes(1024))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)             # the hold kernel carries its own time limit
        for name, call in (("msm_amd_poseidon_permute_device", lambda: c2.poseidon_permute_device(h, d, 5, d_o)),
                           ("msm_amd_poseidon_permute", lambda: c2.poseidon_permute(h, data, 5)),
                           ("msm_amd_poseidon_hash_device", lambda: c2.poseidon_hash_device(h, d, 8, d_o)),
                           ("msm_amd_poseidon_hash", lambda: c2.poseidon_hash(h, data, 8)),
                           ("msm_amd_poseidon_merkle_build_device", lambda: c2.poseidon_merkle_build_device(h, d, 16, d_o)),
                           ("msm_amd_poseidon_merkle_build", lambda: c2.poseidon_merkle_build(h, data, 16)),
                           ("msm_amd_poseidon_merkle_paths_device", lambda: c2.poseidon_merkle_paths_device(h, d, 16, d_o, [3], d_o + 512)),
                           ("msm_amd_poseidon_merkle_paths", lambda: c2.poseidon_merkle_paths(h, data, 16, bytes(15 * 32), [3]))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert c2.to_host(d, len(data)) == data and c2.to_host(d_o, 1024) == bytes(1024)     # the refused calls wrote nothing
        A, M = m.constants(3)
        levels = m.tree(values, 3, A, M, m.R_F, m.R_P[3])
        root, _ = c2.poseidon_merkle_build_device(h, d, 16, d_o)
        assert root == m.enc(levels[-1][0], layout) and c2.to_host(d_o, 15 * 32) == m.pack(m.flat(levels), layout)
        assert c2.poseidon_hash(h, data, 8) == m.pack(levels[0], layout)
        c2.free(d)
        c2.free(d_o)
    finally:
        c2.close()


def test_argument_errors_and_empty_calls(cfg, msm_pkg, dev, params):
    L, vp = msm_pkg.lib(), ctypes.c_void_p
    be32 = msm_pkg.SCALAR_CANON_BE32
    data = m.pack(m.random_values(7, 32), m.MONT_LE)
    d_in, d_out = dev.put(data), dev.put(b"\xA5" * len(data))
    h, h2, h3, h4 = cfg.h, params[2].h, params[3].h, params[4].h
    i_, o_ = vp(d_in), vp(d_out)
    idx, bad = (ctypes.c_uint64 * 2)(0, 7), (ctypes.c_uint64 * 2)(0, 8)
    hout, root = ctypes.create_string_buffer(len(data)), ctypes.create_string_buffer(32)
    per = lambda *a: ("msm_amd_poseidon_permute_device", L.msm_amd_poseidon_permute_device(h, *a, None))                   # noqa: E731
    hsh = lambda *a: ("msm_amd_poseidon_hash_device", L.msm_amd_poseidon_hash_device(h, *a, None))                         # noqa: E731
    bld = lambda *a: ("msm_amd_poseidon_merkle_build_device", L.msm_amd_poseidon_merkle_build_device(h, *a, None))         # noqa: E731
    pth = lambda *a: ("msm_amd_poseidon_merkle_paths_device", L.msm_amd_poseidon_merkle_paths_device(h, *a, None))         # noqa: E731
    hper = lambda *a: ("msm_amd_poseidon_permute", L.msm_amd_poseidon_permute(h, *a))                                      # noqa: E731
    hhsh = lambda *a: ("msm_amd_poseidon_hash", L.msm_amd_poseidon_hash(h, *a))                                            # noqa: E731
    hbld = lambda *a: ("msm_amd_poseidon_merkle_build", L.msm_amd_poseidon_merkle_build(h, *a))                            # noqa: E731
    hpth = lambda *a: ("msm_amd_poseidon_merkle_paths", L.msm_amd_poseidon_merkle_paths(h, *a))                            # noqa: E731
    cases = [
        lambda: per(h3, be32, i_, 2, o_), lambda: per(h3, 7, i_, 2, o_), lambda: hsh(h3, be32, None, i_, 2, o_),           # layout
        lambda: bld(h3, be32, None, i_, 8, o_, root), lambda: pth(h3, be32, i_, 8, vp(d_in + 512), idx, 2, o_),
        lambda: hper(h3, be32, data, 2, hout), lambda: hhsh(h3, 9, None, data, 2, hout),
        lambda: hbld(h3, be32, None, data, 8, hout, root), lambda: hpth(h3, be32, data, 8, data[512:], idx, 2, hout),
        lambda: per(h3, 0, i_, 1 << 32, o_), lambda: hsh(h3, 0, None, i_, 1 << 32, o_),                                    # counts
        lambda: bld(h3, 0, None, i_, 1 << 32, o_, root), lambda: bld(h3, 0, None, i_, 12, o_, root),
        lambda: bld(h3, 0, None, i_, 0, o_, root), lambda: bld(h3, 0, None, i_, 1, o_, root), lambda: bld(h4, 0, None, i_, 8, o_, root),
        lambda: bld(h2, 0, None, i_, 2, o_, root), lambda: hbld(h2, 0, None, data, 4, hout, root),                         # t = 2: no tree
        lambda: pth(h2, 0, i_, 2, vp(d_in + 512), idx, 1, o_), lambda: pth(h3, 0, i_, 12, vp(d_in + 512), idx, 2, o_),
        lambda: pth(h3, 0, i_, 8, vp(d_in + 512), idx, 1 << 31, o_),
        lambda: pth(h3, 0, i_, 8, vp(d_in + 512), bad, 2, o_), lambda: hpth(h3, 0, data, 8, data[512:], bad, 2, hout),     # an index = n_leaves
        lambda: per(h3, 0, None, 2, o_), lambda: per(h3, 0, i_, 2, None), lambda: hsh(h3, 0, None, None, 2, o_),           # null pointers
        lambda: hsh(h3, 0, None, i_, 2, None), lambda: bld(h3, 0, None, None, 8, o_, root), lambda: bld(h3, 0, None, i_, 8, None, root),
        lambda: pth(h3, 0, None, 8, vp(d_in + 512), idx, 2, o_), lambda: pth(h3, 0, i_, 8, None, idx, 2, o_),
        lambda: pth(h3, 0, i_, 8, vp(d_in + 512), None, 2, o_), lambda: pth(h3, 0, i_, 8, vp(d_in + 512), idx, 2, None),
        lambda: hper(h3, 0, None, 2, hout), lambda: hhsh(h3, 0, None, data, 2, None), lambda: hbld(h3, 0, None, data, 8, None, root),
        lambda: per(h3, 0, vp(d_in + 8), 2, o_), lambda: per(h3, 0, i_, 2, vp(d_out + 4)),                                 # alignment
        lambda: hsh(h3, 0, None, vp(d_in + 8), 2, o_), lambda: hsh(h3, 0, None, i_, 2, vp(d_out + 8)),
        lambda: bld(h3, 0, None, vp(d_in + 4), 8, o_, root), lambda: bld(h3, 0, None, i_, 8, vp(d_out + 8), root),
        lambda: pth(h3, 0, i_, 8, vp(d_in + 520), idx, 2, o_), lambda: pth(h3, 0, i_, 8, vp(d_in + 512), idx, 2, vp(d_out + 8)),
        lambda: per(h3, 0, i_, 2, vp(d_in + 32)), lambda: per(h3, 0, vp(d_in + 32), 2, i_),                                # overlap
        lambda: hsh(h3, 0, None, i_, 4, i_), lambda: hsh(h3, 0, None, i_, 4, vp(d_in + 32 * 7)),
        lambda: hsh(h3, 0, None, vp(d_in + 32 * 3), 4, i_), lambda: hsh(h2, 0, None, i_, 4, vp(d_in + 32)),
        lambda: bld(h3, 0, None, i_, 8, i_, root), lambda: bld(h3, 0, None, i_, 8, vp(d_in + 32 * 7), root),
        lambda: bld(h3, 0, None, vp(d_in + 32 * 6), 8, i_, root),
        lambda: pth(h3, 0, i_, 8, vp(d_in + 512), idx, 2, vp(d_in + 32 * 7)), lambda: pth(h3, 0, i_, 8, vp(d_in + 512), idx, 2, vp(d_in + 512 + 32 * 6)),
    ]
    for j, case in enumerate(cases):
        name, st = case()
        assert st == msm_pkg.INPUT_ERROR, (j, name)
        assert name.encode() + b":" in L.msm_amd_last_error(h), (j, name, L.msm_amd_last_error(h))
    assert dev.get(d_out, len(data)) == b"\xA5" * len(data) and dev.get(d_in, len(data)) == data
    assert hout.raw == bytes(len(data)) and root.raw == bytes(32)
    # nothing to do: OK, nothing touched
    assert per(h3, 0, None, 0, None)[1] == msm_pkg.OK and hsh(h3, 0, None, None, 0, None)[1] == msm_pkg.OK
    assert hper(h3, 0, None, 0, None)[1] == msm_pkg.OK and hhsh(h3, 0, None, None, 0, None)[1] == msm_pkg.OK
    assert pth(h3, 0, i_, 8, vp(d_in + 512), None, 0, None)[1] == msm_pkg.OK and hpth(h3, 0, data, 8, data[512:], None, 0, None)[1] == msm_pkg.OK
    assert dev.get(d_out, len(data)) == b"\xA5" * len(data)
    # digests right behind the input are disjoint from it; so is a tree right behind its leaves
    assert hsh(h3, 0, None, i_, 4, vp(d_in + 32 * 8))[1] == msm_pkg.OK
    assert dev.get(d_in + 32 * 8, 32 * 4) == msm_pkg.host_poseidon_hash(*shape(msm_pkg, 3), data[:32 * 8], 4)
    assert bld(h3, 0, None, i_, 8, vp(d_in + 32 * 8), root)[1] == msm_pkg.OK
    assert (dev.get(d_in + 32 * 8, 32 * 7), root.raw) == msm_pkg.host_poseidon_merkle_build(*shape(msm_pkg, 3), data[:32 * 8], 8)
