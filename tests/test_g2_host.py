"""CPU-only tests of the BN254 G2 MSM: the big-integer model itself (tests/g2_ref.py), the library's CPU G2 MSM
against a naive sum, the progression generator, the layouts and error paths, the raw-limb G2 arithmetic of the device
kernels (run here through its host twin) against big integers at the edges of its bounds contract, the bounds model
and the register use of the G2 kernels."""
import os
import random
import subprocess

import pytest

import g2_ref as g
from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc")


# ---- the model ------------------------------------------------------------------------------------------------------
def test_oracle_twist_and_generator():
    assert g.B_TWIST == g.mul2((3, 0), g.inv2((9, 1)))
    assert g.mul2(g.B_TWIST, (9, 1)) == (3, 0)
    assert g.on_curve(g.GEN2)
    assert g.scalar_mul(g.R_ORDER, g.GEN2) is None
    assert g.scalar_mul(g.R_ORDER - 1, g.GEN2) == g.neg(g.GEN2)
    p5 = g.scalar_mul(5, g.GEN2)
    assert p5 == g.add(g.add(g.add(g.GEN2, g.GEN2), g.add(g.GEN2, g.GEN2)), g.GEN2) and g.on_curve(p5)


# ---- CPU G2 MSM against a naive sum ---------------------------------------------------------------------------------
_DLOGS = {}


def _point(a):
    """a G2 (cached): the bases of the MSM cases, with their discrete logs known"""
    a %= g.R_ORDER
    if a not in _DLOGS:
        _DLOGS[a] = g.scalar_mul(a, g.GEN2)
    return _DLOGS[a]


def msm_case(n, seed):
    """(scalars, dlogs) with the adversarial entries of a small case: identity bases (dlog 0), zero scalars, scalar
    r - 1, a repeated base (P, P) and an opposite pair (P, -P)"""
    rng = random.Random(seed)
    dl = [rng.randrange(1, 1 << 40) for _ in range(n)]
    ks = [rng.randrange(g.R_ORDER) for _ in range(n)]
    if n >= 3:
        dl[1] = 0                      # identity base
        ks[2] = 0                      # zero scalar
        ks[0] = g.R_ORDER - 1
    if n >= 17:
        dl[5] = dl[4]                  # (P, P)
        dl[7] = -dl[6] % g.R_ORDER     # (P, -P)
        ks[7] = ks[6]
        dl[9] = 0
        ks[9] = g.R_ORDER - 1
    return ks, dl


def encode_case(ks, dl, scalar_layout, point_layout):
    enc = g.encode_h2c if point_layout == 0 else g.encode_ark
    pts = b"".join(enc(_point(a) if a else None) for a in dl)
    sc = b"".join(g.encode_scalar(k, scalar_layout) for k in ks)
    return sc, pts


def expected(ks, dl):
    return g.scalar_mul(sum(k * a for k, a in zip(ks, dl)) % g.R_ORDER, g.GEN2)


def assert_result(out, exp):
    assert len(out) == 192
    if exp is None:
        assert out == g.identity_bytes()
        return
    assert g.decode_jacobian(out) == exp
    assert out[128:] == g.identity_bytes()[:64]     # z = (R mod p, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 257])
def test_host_msm_g2_against_naive(msm_pkg, n):
    ks, dl = msm_case(n, 1000 + n)
    exp = expected(ks, dl)
    for sl, pl in ((0, 0), (1, 1), (0, 1), (1, 0), (2, 0)):
        sc, pts = encode_case(ks, dl, sl, pl)
        out = msm_pkg.host_msm_g2(sc, pts, n, threads=4, scalar_layout=sl, point_layout=pl)
        assert_result(out, exp)


def test_host_msm_g2_naive_sum_model():
    """the model's naive sum and the discrete-log shortcut of the MSM tests agree"""
    ks, dl = msm_case(17, 7)
    pts = [_point(a) if a else None for a in dl]
    assert g.msm_naive(ks, pts) == expected(ks, dl)


def test_host_msm_g2_empty_and_cancelling(msm_pkg):
    assert msm_pkg.host_msm_g2(b"", b"", 0) == g.identity_bytes()
    p = _point(12345)
    sc = g.encode_scalar(77, 0) * 2
    out = msm_pkg.host_msm_g2(sc, g.encode_h2c(p) + g.encode_h2c(g.neg(p)), 2)
    assert out == g.identity_bytes()


def test_g2_point_bytes_and_input_errors(msm_pkg):
    assert msm_pkg.g2_point_bytes(msm_pkg.G2_POINT_H2C_AFFINE) == 128
    assert msm_pkg.g2_point_bytes(msm_pkg.G2_POINT_ARK_AFFINE) == 136
    assert msm_pkg.g2_point_bytes(7) == 0
    with pytest.raises(msm_pkg.MsmError) as e:
        msm_pkg.host_msm_g2(bytes(32), bytes(128), 1, point_layout=7)
    assert e.value.status == msm_pkg.INPUT_ERROR
    with pytest.raises(msm_pkg.MsmError) as e:
        msm_pkg.host_msm_g2(bytes(32), bytes(128), 1, scalar_layout=9)
    assert e.value.status == msm_pkg.INPUT_ERROR
    L = msm_pkg.lib()
    out = bytes(192)
    assert L.msm_amd_host_msm_g2(0, 0, None, None, 5, 1, out) == msm_pkg.INPUT_ERROR


def test_g2_progression(msm_pkg):
    a0, d = 987654321, 123456789
    n = 3000
    pts = msm_pkg.g2_progression(g.encode_h2c(_point(a0)), g.encode_h2c(_point(d)), n, threads=3)
    assert len(pts) == 128 * n
    for i in (0, 1, 2, 999, 1000, 1001, 2047, n - 1):
        assert g.decode_h2c(pts[128 * i:128 * i + 128]) == g.scalar_mul(a0 + i * d, g.GEN2), i
    # through the identity: start = -step
    pts = msm_pkg.g2_progression(g.encode_h2c(g.neg(_point(d))), g.encode_h2c(_point(d)), 3, threads=1)
    assert pts[128:256] == bytes(128)
    assert g.decode_h2c(pts[256:]) == _point(d)


# ---- raw-limb G2 arithmetic (host twin of the device kernels) -----------------------------------------------------
RP = g.P / g.RHO


def fq2_corpus(seed, n=120):
    """operand pairs at the edges of Fq2::mul's contract: a < 32 p, b0 < 64 p, b1 < 32 p (random multiples, the top one half the
    time), limbs normalised with borrowed limbs at 2^29 + 7"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        a, b = g.rand_fq2(rng), g.rand_fq2(rng)
        if i % 10 == 0:
            a = (0, a[1])
        ma = (rng.choice([1, 2, 20, 31]), rng.choice([1, 2, 20, 31]))
        mb = (rng.choice([1, 4, 20, 63]), rng.choice([1, 4, 20, 31]))
        out.append((g.fq2_rec(a, ma, rng), g.fq2_rec(b, mb, rng)))
    return out


def check_fq2(op, aw, bw, ow):
    A0, A1 = g.value(aw[:9]), g.value(aw[9:18])
    B0, B1 = g.value(bw[:9]), g.value(bw[9:18])
    C0, C1 = g.value(ow[:9]), g.value(ow[9:18])
    if op == 0:
        e0, e1 = A0 * B0 - A1 * B1, A0 * B1 + A1 * B0
        b0 = 1 + RP * (A0 / g.P * B0 / g.P + 32 * A1 / g.P)
        b1 = 1 + RP * (A0 / g.P * B1 / g.P + A1 / g.P * B0 / g.P)
    else:
        e0, e1 = A0 * A0 - A1 * A1, 2 * A0 * A1
        b0 = 1 + RP * (A0 + A1) / g.P * (A0 / g.P + 32)
        b1 = 1 + RP * 2 * A0 / g.P * A1 / g.P
    assert (C0 - e0 * g.RHO_INV) % g.P == 0 and (C1 - e1 * g.RHO_INV) % g.P == 0
    assert C0 < b0 * g.P and C1 < b1 * g.P
    assert all(ow[k] < (1 << 29) for k in list(range(8)) + list(range(9, 17)))


@pytest.mark.parametrize("op", [0, 1])
def test_raw_fq2_ops_host(msm_pkg, op):
    cases = fq2_corpus(10 + op)
    a = [w for x, _ in cases for w in g.pad(x)]
    b = [w for _, y in cases for w in g.pad(y)]
    out = msm_pkg.test_op_g2_host(op, a, b, len(cases))
    for i, (x, y) in enumerate(cases):
        check_fq2(op, x, y, out[80 * i:80 * i + 80])


def point_corpus(op, seed, n=12):
    """(a words, b words, expected affine, expected vanished) for the point ops, ordinary and exceptional cases"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        p = _point(rng.randrange(1, 1 << 60))
        kind = ("plain", "equal", "opposite")[i % 3]
        q = _point(rng.randrange(1, 1 << 60)) if kind == "plain" else (p if kind == "equal" else g.neg(p))
        if op == g_ops.MADD:
            neg_b = i % 2 == 1
            bw, qv = g.aff_rec(g.neg(q) if neg_b else q, rng, negated=neg_b)
            exp = g.add(p, qv)
            out.append((g.xyzz_rec(p, rng), g.pad(bw), exp, kind == "opposite"))
        elif op == g_ops.MMADD:
            if i % 4 == 1:   # p's y in the negated limb form (4 p - y of -p)
                aw, pv = g.aff_rec(g.neg(p), rng, negated=True)
            else:
                aw, pv = g.aff_rec(p, rng)
            bw, qv = g.aff_rec(q, rng)
            out.append((g.pad(aw), g.pad(bw), g.add(pv, qv), kind == "opposite"))
        elif op in (g_ops.ADD_NZ, g_ops.ADD):
            out.append((g.xyzz_rec(p, rng), g.xyzz_rec(q, rng), g.add(p, q), op == g_ops.ADD_NZ and kind == "opposite"))
        else:
            out.append((g.xyzz_rec(p, rng), [0] * 72, g.add(p, p), False))
    return out


class g_ops:
    MADD, MMADD, ADD_NZ, ADD, DOUBLE = 2, 3, 4, 5, 6


POINT_OPS = [g_ops.MADD, g_ops.MMADD, g_ops.ADD_NZ, g_ops.ADD, g_ops.DOUBLE]


def check_point(ow, exp, vanished):
    assert g.decode_xyzz(ow[:72]) == exp
    assert ow[72] == (1 if vanished else 0)
    if exp is not None:
        m = g.component_multiples(ow, 8)
        assert max(m[0:2]) < 1.21 and max(m[2:4]) < 13.4 and max(m[4:6]) < 3.2 and max(m[6:8]) < 2.04, m
        assert g.normalised(ow, 8)


@pytest.mark.parametrize("op", POINT_OPS)
def test_raw_point_ops_host(msm_pkg, op):
    cases = point_corpus(op, 50 + op)
    a = [w for c in cases for w in c[0]]
    b = [w for c in cases for w in c[1]]
    out = msm_pkg.test_op_g2_host(op, a, b, len(cases))
    for i, (_, _, exp, van) in enumerate(cases):
        check_point(out[80 * i:80 * i + 80], exp, van)


def test_raw_point_add_identity_operands(msm_pkg):
    rng = random.Random(3)
    p = _point(99)
    ident = [0] * 72
    ident[0:9] = g.limbs_of(g.RHO % g.P)
    ident[18:27] = g.limbs_of(g.RHO % g.P)
    pw = g.xyzz_rec(p, rng)
    out = msm_pkg.test_op_g2_host(g_ops.ADD, pw + ident, ident + pw, 2)
    assert out[:72] == pw and out[80:152] == pw


# ---- bounds model and register use ----------------------------------------------------------------------------------
def test_g2_bounds_model():
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "g2_bounds.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "invariant" in r.stdout


def _device_notes(obj):
    """kernel metadata of the gfx950 code object inside a hipcc object file"""
    import shutil
    import tempfile
    llvm = "/opt/rocm/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools) or not os.path.exists(obj):
        pytest.skip("ROCm LLVM tools or the built object are missing")
    d = tempfile.mkdtemp()
    try:
        fat, dev = os.path.join(d, "fat.bin"), os.path.join(d, "dev.o")
        subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy.o")])
        subprocess.check_call([tools[1], "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
        return subprocess.check_output([tools[2], "--notes", dev], text=True)
    finally:
        shutil.rmtree(d)


def kernel_scratch(obj):
    """private segment (scratch) bytes per kernel of the gfx950 code object inside a hipcc object file"""
    kernels, name = {}, None
    for line in _device_notes(obj).splitlines():
        s = line.strip().lstrip("- ")
        if s.startswith(".name:"):
            name = s.split(":", 1)[1].strip()
        elif s.startswith(".private_segment_fixed_size:") and name:
            kernels[name] = int(s.split(":", 1)[1])
    return kernels


def test_g2_kernels_use_no_scratch():
    kernels = kernel_scratch(os.path.join(CSRC, "k_g2.o"))
    g2 = {k: v for k, v in kernels.items() if "_g2_kernel" in k}
    assert len(g2) >= 7, kernels
    assert all(v == 0 for v in g2.values()), g2
