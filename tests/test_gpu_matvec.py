"""The sparse product on the GPU (msm_amd_fr_matrix_*, msm_amd_fr_matvec*) against the host twin and the big-integer model
of tests/matvec_ref.py (tests/test_matvec_host.py pins the twin and the planner to the model on the CPU).  Every
comparison is of bytes: device call = host-buffer call = twin = model.  Rows of at most LONG entries take one lane each,
longer rows one wave per segment of SEG entries, rows of several segments a fold launch: MSM_AMD_FR_MAT_LONG and
MSM_AMD_FR_MAT_SEG_LOG bring all three down to matrices of a few hundred entries, MSM_AMD_FR_MAT_SIGNS selects the kernels
that skip the product for the values 1 and r - 1."""
import random

import numpy as np
import pytest

import matvec_ref as m
import ntt_ref

pytestmark = pytest.mark.gpu

R = m.R
PAIRS = [(v, c) for v in m.LAYOUTS for c in m.LAYOUTS]     # (layout of the values, layout of x and y)


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


@pytest.fixture(params=[0, 1], ids=["products", "signs"])
def small_knobs(msm_pkg, monkeypatch, request):
    """a ctx of its own whose rows above 4 entries take the wave path in segments of 64; with both forms of the kernels
    (MSM_AMD_FR_MAT_SIGNS: values 1 and r - 1 are added and subtracted without a product)"""
    monkeypatch.setenv("MSM_AMD_FR_MAT_LONG", "4")
    monkeypatch.setenv("MSM_AMD_FR_MAT_SEG_LOG", "6")
    monkeypatch.setenv("MSM_AMD_FR_MAT_SIGNS", str(request.param))
    c2 = msm_pkg.setup_metal_state()
    yield c2
    c2.close()


def check(cfg, msm_pkg, mat, x, v_layout, layout, tag, exp=None, n_distinct=None):
    """device call = host-buffer call = twin = model; y starts as 0xFF bytes, x and the handle are left as they were"""
    if exp is None:
        exp = m.matvec(mat, x, v_layout, layout)
    values_l = mat.values if v_layout == layout else m.recode(mat.values, v_layout, layout)
    args = mat.c_args()
    assert m.first_difference(msm_pkg.host_fr_matvec(*args[:4], values_l, x, layout), exp) is None, tag
    dev = Device(cfg)
    h = cfg.fr_matrix_build(*args, v_layout)
    try:
        info = h.info()
        assert (info["n_rows"], info["n_cols"], info["nnz"]) == (mat.n_rows, mat.n_cols, mat.nnz), tag
        assert info["device_bytes"] >= 4 * (mat.n_rows + 1) + 8 * mat.nnz + 32 * info["n_distinct"], tag
        if n_distinct is not None:
            assert info["n_distinct"] == n_distinct, tag
        d_x, d_y = dev.put(x), dev.put(b"\xFF" * (32 * mat.n_rows))
        assert cfg.fr_matvec_device(h, d_x, d_y, layout) >= 0
        assert m.first_difference(dev.get(d_y, 32 * mat.n_rows), exp) is None, tag
        assert dev.get(d_x, len(x)) == x, tag
        assert cfg.fr_matvec(h, x, layout) == exp, tag
        assert h.info() == info, tag
        cfg.to_device(d_y, b"\xFF" * (32 * mat.n_rows))          # the handle serves a second product
        cfg.fr_matvec_device(h, d_x, d_y, layout)
        assert dev.get(d_y, 32 * mat.n_rows) == exp, tag
    finally:
        h.free()
        dev.close()
    return info


# ---- 1. the lane path at the default knobs -----------------------------------------------------------------------------------
def lane_lengths(n_rows, seed):
    """0 .. 8 entries mixed inside a wave; the first and the last row empty; rows 64 .. 127 empty (a whole idle wave)"""
    rng = random.Random(seed)
    lengths = [rng.randrange(9) for _ in range(n_rows)]
    lengths[0] = lengths[-1] = 0
    if n_rows > 3:
        lengths[1], lengths[-2] = 8, 7
    for i in range(64, min(128, n_rows)):
        lengths[i] = 0
    return lengths


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_lane_path(cfg, msm_pkg, n_rows):
    n_cols = 97
    lengths = lane_lengths(n_rows, n_rows)
    assert msm_pkg.test_fr_matrix_plan(m.from_lengths(0, lengths, n_cols, 0).row_ptr)["launches"] == 1
    for v_layout, layout in PAIRS:
        mat = m.from_lengths(n_rows + v_layout, lengths, n_cols, v_layout)
        x = m.encode(m.random_values(7 * n_rows + layout, n_cols), layout)
        check(cfg, msm_pkg, mat, x, v_layout, layout, (n_rows, v_layout, layout))
    if n_rows == 1:    # the one row with entries
        mat = m.from_lengths(5, [6], n_cols, m.MONT_LE)
        check(cfg, msm_pkg, mat, m.encode(m.random_values(8, n_cols), m.CANON_LE), m.MONT_LE, m.CANON_LE, "one row")


# ---- 2. the wave path and the fold ------------------------------------------------------------------------------------------
WAVE_LENGTHS = [5, 63, 64, 65, 127, 128, 129, 200, 256]


def test_wave_path(small_knobs, msm_pkg):
    c2 = small_knobs
    n_cols = 301
    rng = random.Random(9)
    mixed = []                                               # long and short rows inside one 64-row group
    for i in range(64):
        mixed.append(WAVE_LENGTHS[i // 2 % len(WAVE_LENGTHS)] if i & 1 else rng.randrange(5))
    cases = {
        "every length": ([0, 3] + WAVE_LENGTHS + [1, 0], 3),
        "split rows first, adjacent and last": ([129, 200, 3, 0, 2, 65, 4, 256], 3),
        "long rows only": ([65, 64, 5, 130], 3),
        "one long row": ([200], 3),
        "one row of one segment": ([64], 2),
        "no split row": ([5, 63, 64, 3, 0, 64, 4, 5], 2),
        "mixed group": (mixed, 3),
    }
    for name, (lengths, launches) in cases.items():
        probe = m.from_lengths(0, lengths, n_cols, m.MONT_LE)
        plan = msm_pkg.test_fr_matrix_plan(probe.row_ptr, 4, 6)
        assert plan["launches"] == launches, name
        assert plan["wave_rows"] == sum(1 for ln in lengths if ln > 4), name
        for v_layout, layout in PAIRS if name in ("every length", "mixed group") else PAIRS[1:3]:
            mat = m.from_lengths(len(lengths) + v_layout, lengths, n_cols, v_layout)
            x = m.encode(m.random_values(len(lengths) + 10 * layout, n_cols), layout)
            check(c2, msm_pkg, mat, x, v_layout, layout, (name, v_layout, layout))


# ---- 3. the dictionary ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v_layout", m.LAYOUTS)
def test_dictionary(cfg, small_knobs, msm_pkg, v_layout):
    n_cols = 40
    lengths = [3, 0, 70, 2, 4, 150, 1]
    x = m.encode(m.random_values(3, n_cols), m.MONT_LE)
    nnz = sum(lengths)
    for ctx in (cfg, small_knobs):                           # the lane path alone; lane, wave and fold
        one = m.from_lengths(1, lengths, n_cols, v_layout, values=[12345])
        assert check(ctx, msm_pkg, one, x, v_layout, m.MONT_LE, "one value", n_distinct=1)["n_distinct"] == 1
        distinct = m.from_lengths(2, lengths, n_cols, v_layout, values=list(range(1000, 1000 + nnz)))
        check(ctx, msm_pkg, distinct, x, v_layout, m.MONT_LE, "all distinct", n_distinct=nnz)
        signs = m.from_lengths(3, lengths, n_cols, v_layout, values=[1, R - 1, 1, 1, R - 1])
        check(ctx, msm_pkg, signs, x, v_layout, m.CANON_LE if v_layout == m.MONT_LE else m.MONT_LE, "rows of +-1",
              n_distinct=2)
        zeros = m.from_lengths(4, lengths, n_cols, v_layout, values=[0, 5, 0, 0, 7, 0])
        check(ctx, msm_pkg, zeros, x, v_layout, m.MONT_LE, "explicit zeros", n_distinct=3)
        # the raw words: r reads as 0 (and, canonical, r + 1 as 1), so seven records are fewer residues
        recs = m.edge_records(v_layout)
        raw_mat = m.from_lengths(5, lengths, n_cols, v_layout)
        raw_mat.values = b"".join(recs[k % len(recs)] for k in range(nnz))
        residues = m.n_distinct(raw_mat, v_layout)           # Montgomery: the word r + 1 is not the record of 1
        assert residues == (6 if v_layout == m.MONT_LE else 5)
        xr = b"".join(m.edge_records(m.CANON_LE)[k % 7] for k in range(n_cols))
        check(ctx, msm_pkg, raw_mat, xr, v_layout, m.CANON_LE, "raw words", n_distinct=residues)


def test_sign_kernels_at_the_default_knobs(msm_pkg, monkeypatch):
    """the lane path of the other form: signs and other values mixed inside a wave, every layout pair"""
    monkeypatch.setenv("MSM_AMD_FR_MAT_SIGNS", "1")
    c2 = msm_pkg.setup_metal_state()
    try:
        lengths = lane_lengths(257, 3)
        x_cols = 60
        for v_layout, layout in PAIRS:
            mixed = m.from_lengths(40 + v_layout, lengths, x_cols, v_layout, values=[1, R - 1, 77, 1, 0, R - 1, R - 2, 2])
            x = m.encode(m.random_values(41 + layout, x_cols), layout)
            check(c2, msm_pkg, mixed, x, v_layout, layout, ("mixed", v_layout, layout), n_distinct=6)
        only = m.from_lengths(42, lengths, x_cols, m.MONT_LE, values=[R - 1])
        check(c2, msm_pkg, only, x, m.MONT_LE, m.CANON_LE, "minus one only", n_distinct=1)
    finally:
        c2.close()


# ---- 4. larger -------------------------------------------------------------------------------------------------------------------
def test_r1cs_shape_at_2_18(cfg, msm_pkg):
    """against the twin (bytes), a closed form, and the model on 1 000 sampled rows"""
    n = 1 << 18
    mat = m.r1cs_shape(4, n)
    plan = msm_pkg.test_fr_matrix_plan(mat.row_ptr.tobytes())
    assert plan["wave_rows"] >= n // 1000 and plan["split_rows"] >= 1 and plan["launches"] == 3
    x = np.random.default_rng(5).bytes(32 * n)              # any 256-bit word is a record
    args = mat.c_args()
    dev = Device(cfg)
    h = cfg.fr_matrix_build(*args, m.MONT_LE)
    try:
        assert h.info()["n_distinct"] == 32
        d_x, d_y = dev.put(x), dev.put(b"\xFF" * (32 * n))
        cfg.fr_matvec_device(h, d_x, d_y, m.MONT_LE)
        got = dev.get(d_y, 32 * n)
        assert m.first_difference(got, msm_pkg.host_fr_matvec(*args, x, m.MONT_LE)) is None
        rows = sorted(set(random.Random(6).sample(range(n), 997)) | {0, n // 2, n - 1})
        rows += [int(i) for i in np.flatnonzero(np.diff(mat.row_ptr.astype(np.int64)) == 1000)[:3]]
        exp = m.encode(m.rows_model(mat, x, m.MONT_LE, m.MONT_LE, rows), m.MONT_LE)
        assert m.first_difference(b"".join(got[32 * i:32 * i + 32] for i in rows), exp) is None
        h.free()
        # closed form: every value 1 and x[j] = j + 1, canonical records: y[i] = the sum of (column + 1) over the row
        ones = m.r1cs_shape(4, n, ones=True)
        h = cfg.fr_matrix_build(*ones.c_args(), m.MONT_LE)
        assert h.info()["n_distinct"] == 1
        cfg.to_device(d_x, b"".join((j + 1).to_bytes(32, "little") for j in range(n)))
        cfg.fr_matvec_device(h, d_x, d_y, m.CANON_LE)
        sums = np.add.reduceat(ones.col_idx.astype(np.uint64) + 1, ones.row_ptr[:-1].astype(np.int64))   # no row is empty
        exp = b"".join(int(v).to_bytes(32, "little") for v in sums)
        assert m.first_difference(dev.get(d_y, 32 * n), exp) is None
    finally:
        h.free()
        dev.close()


# ---- 5. stale workspaces, a busy ctx, arguments, handles ---------------------------------------------------------------------
def test_poisoned_workspaces_and_bounded_wait(small_knobs, msm_pkg):
    c2 = small_knobs
    lengths = [3, 200, 0, 129, 64, 2]
    mat = m.from_lengths(21, lengths, 50, m.MONT_LE)
    x = m.encode(m.random_values(22, 50), m.MONT_LE)
    exp = m.matvec(mat, x, m.MONT_LE, m.MONT_LE)
    dev = Device(c2)
    h = c2.fr_matrix_build(*mat.c_args(), m.MONT_LE)
    try:
        assert msm_pkg.test_fr_matrix_plan(mat.row_ptr, 4, 6)["partials"] == 7
        d_x, d_y = dev.put(x), dev.put(b"\xFF" * (32 * 6))
        c2.fr_matvec_device(h, d_x, d_y)                     # sizes the partials
        for byte in (0xFF, 0x00, 0x5A):
            c2.test_fill_workspaces(byte)
            c2.to_device(d_y, bytes([byte ^ 0xFF]) * (32 * 6))
            c2.fr_matvec_device(h, d_x, d_y)
            assert dev.get(d_y, 32 * 6) == exp, byte
            c2.test_fill_workspaces(byte)
            assert c2.fr_matvec(h, x) == exp, byte
        c2.to_device(d_y, b"\xEE" * (32 * 6))
        c2.set_wait_timeout_ms(150)
        hold = c2.test_hold(4000)                            # the hold kernel carries its own time limit
        for name, call in (("msm_amd_fr_matvec_device", lambda: c2.fr_matvec_device(h, d_x, d_y)),
                           ("msm_amd_fr_matvec", lambda: c2.fr_matvec(h, x, n_rows=6))):
            with pytest.raises(msm_pkg.MsmError) as e:
                call()
            assert e.value.status == msm_pkg.PIPELINE_ERROR and name in str(e.value), e.value
        c2.test_release(hold)
        c2.set_wait_timeout_ms(60000)
        c2.synchronize()
        assert dev.get(d_y, 32 * 6) == b"\xEE" * (32 * 6)    # the refused calls wrote nothing
        c2.fr_matvec_device(h, d_x, d_y)
        assert dev.get(d_y, 32 * 6) == exp and c2.fr_matvec(h, x) == exp
    finally:
        h.free()
        dev.close()


def test_argument_errors_and_handles(cfg, msm_pkg, dev):
    mat = m.from_lengths(31, [2, 0, 3], 4, m.MONT_LE)
    x = m.encode([1, 2, 3, 4], m.MONT_LE)
    exp = m.matvec(mat, x, m.MONT_LE, m.MONT_LE)

    def refused(fn, *a, **kw):
        with pytest.raises(msm_pkg.MsmError) as e:
            fn(*a, **kw)
        assert e.value.status == msm_pkg.INPUT_ERROR, (a, kw)

    build = lambda **kw: cfg.fr_matrix_build(**dict(dict(n_rows=3, n_cols=4, row_ptr=mat.row_ptr, col_idx=mat.col_idx,   # noqa: E731
                                                         values=mat.values, scalar_layout=m.MONT_LE), **kw))
    refused(build, scalar_layout=msm_pkg.SCALAR_CANON_BE32)
    refused(build, n_rows=0, row_ptr=[0])
    refused(build, n_cols=0)
    refused(build, n_rows=1 << 32)
    refused(build, n_cols=1 << 32)
    refused(build, row_ptr=None)
    refused(build, col_idx=None)
    refused(build, values=None)
    refused(build, row_ptr=[1, 2, 2, 5])
    refused(build, row_ptr=[0, 2, 1, 5])
    refused(build, row_ptr=[0, 2, 2, 1 << 32])
    refused(build, col_idx=[0, 1, 2, 4, 3])                  # a column equal to n_cols
    refused(build, col_idx=[0, 1, 2, 3, 0xFFFFFFFF])
    empty = cfg.fr_matrix_build(3, 4, [0, 0, 0, 0], None, None)    # nnz = 0 without arrays
    assert empty.info()["nnz"] == 0 and empty.info()["n_distinct"] == 0
    assert cfg.fr_matvec(empty, x) == bytes(32 * 3)
    empty.free()

    h, h2 = build(), build(values=m.recode(mat.values, m.MONT_LE, m.CANON_LE), scalar_layout=m.CANON_LE)   # two live matrices
    dom = cfg.ntt_domain(ntt_ref.H2C, 4)
    try:
        d = dev.put(x + b"\xDD" * (32 * 4))                  # x, then room for y
        d_y = d + 32 * 4
        assert cfg.fr_matvec_device(h, d, d_y) >= 0 and dev.get(d_y, 32 * 3) == exp
        assert cfg.fr_matvec_device(h2, d, d_y) >= 0 and dev.get(d_y, 32 * 3) == exp
        refused(cfg.fr_matvec_device, h, d, d + 32 * 3)      # y's first record is x's last
        refused(cfg.fr_matvec_device, h, d + 32 * 2, d)      # y's last record is x's first
        refused(cfg.fr_matvec_device, h, d, d)
        refused(cfg.fr_matvec_device, h, d + 8, d_y)         # not 16-byte aligned
        refused(cfg.fr_matvec_device, h, d, d_y + 8)
        refused(cfg.fr_matvec_device, h, 0, d_y)
        refused(cfg.fr_matvec_device, h, d, 0)
        refused(cfg.fr_matvec_device, h, d, d_y, msm_pkg.SCALAR_CANON_BE32)
        refused(cfg.fr_matvec, h, None, n_rows=3)
        refused(cfg.fr_matvec, h, x, msm_pkg.SCALAR_CANON_BE32, n_rows=3)
        refused(cfg.fr_matvec_device, dom, d, d_y)           # a transform domain is no matrix
        refused(cfg.fr_matvec, dom, x, n_rows=3)
        refused(cfg.fr_matrix_info, dom)
        refused(cfg.fr_matrix_free, dom)
        refused(cfg.fr_matvec_device, 0, d, d_y)
        refused(cfg.ntt_device, h.h, d, d)                   # and a matrix no transform domain
        h.free()
        refused(cfg.fr_matvec_device, h, d, d_y)             # a freed handle
        refused(cfg.fr_matvec, h, x, n_rows=3)
        refused(h.info)
        refused(h.free)
        assert cfg.fr_matvec(h2, x) == exp                   # the other matrix lives on
        assert dev.get(d, len(x)) == x
    finally:
        h2.free()
        dom.free()


# ---- 6. the witness map, end to end ----------------------------------------------------------------------------------------------
def test_witness_map_recipe(cfg, msm_pkg, dev):
    """A satisfied R1CS of n - 3 constraints on the domain of n = 2^8: [A; B; C] stacked with empty rows up to n each, one
    product, the inverse and the coset transforms with n_vec = 3, MULSUB_SCALE, the coset inverse -- all on the device."""
    log_n, root = 8, ntt_ref.H2C
    n, rows, free = 1 << 8, (1 << 8) - 3, 40
    rng = random.Random(88)
    z = [1] + [rng.randrange(R) for _ in range(free - 1)] + [0] * rows    # z[free + i] = w_i
    short = lambda seed: m.from_lengths(seed, [rng.randrange(1, 5) for _ in range(rows)], free, m.MONT_LE)   # noqa: E731
    A, B = short(1), short(2)
    A.n_cols = B.n_cols = free + rows
    zr = m.encode(z, m.MONT_LE)
    az, bz = m.rows_model(A, zr, m.MONT_LE, m.MONT_LE, range(rows)), m.rows_model(B, zr, m.MONT_LE, m.MONT_LE, range(rows))
    for i in range(rows):
        z[free + i] = az[i] * bz[i] % R
    zr = m.encode(z, m.MONT_LE)
    C = m.Csr(rows, free + rows, list(range(rows + 1)), [free + i for i in range(rows)], m.encode([1] * rows, m.MONT_LE))
    stacked = m.stack([A, B, C], n)
    abc = m.matvec(stacked, zr, m.MONT_LE, m.MONT_LE)
    a, b, c = (m.decode(abc[32 * n * k:32 * n * (k + 1)], m.MONT_LE) for k in range(3))
    assert all(a[i] * b[i] % R == c[i] for i in range(n)) and any(c)

    g = 7
    g_rec = m.encode([g], m.MONT_LE)
    k_rec = m.encode([pow(pow(g, n, R) - 1, -1, R)], m.MONT_LE)
    h = cfg.fr_matrix_build(*stacked.c_args(), m.MONT_LE)
    dom = cfg.ntt_domain(root, log_n)
    try:
        d_z, d = dev.put(zr), dev.put(b"\xFF" * (32 * 3 * n))
        cfg.fr_matvec_device(h, d_z, d)
        assert dev.get(d, 32 * 3 * n) == abc
        cfg.ntt_device(dom, d, d, msm_pkg.NTT_INVERSE, n_vec=3)
        cfg.ntt_device(dom, d, d, msm_pkg.NTT_FORWARD, shift=g_rec, n_vec=3)
        cfg.fr_map_device(msm_pkg.FR_MULSUB_SCALE, d, d + 32 * n, d + 64 * n, n, d, k=k_rec)
        cfg.ntt_device(dom, d, d, msm_pkg.NTT_INVERSE, shift=g_rec)
        got = dev.get(d, 32 * n)
    finally:
        h.free()
        dom.free()
    # the same with big integers
    coeffs = [ntt_ref.transform(v, root, log_n, ntt_ref.INVERSE) for v in (a, b, c)]
    ea, eb, ec = (ntt_ref.transform(v, root, log_n, ntt_ref.FORWARD, g) for v in coeffs)
    kk = pow(pow(g, n, R) - 1, -1, R)
    hq = ntt_ref.transform([kk * (x * y - w) % R for x, y, w in zip(ea, eb, ec)], root, log_n, ntt_ref.INVERSE, g)
    assert m.first_difference(got, m.encode(hq, m.MONT_LE)) is None
    hc = m.decode(got, m.MONT_LE)
    assert hc[n - 1] == 0 and any(hc)
    tau = rng.randrange(2, R)
    ev = lambda p: sum(v * pow(tau, i, R) for i, v in enumerate(p)) % R   # noqa: E731
    assert (ev(coeffs[0]) * ev(coeffs[1]) - ev(coeffs[2])) % R == ev(hc) * (pow(tau, n, R) - 1) % R
