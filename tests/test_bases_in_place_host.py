"""The caller's G1 bases read in place: the limbs of E << 3 / E << 2 are the coordinates of the same point on the
isomorphic curve E': y'^2 = x'^3 + 3/64 (csrc/bn254_ec29.hip.h).  Here, on the host build of the same headers (the raw
op MSM_AMD_RAW_BASES_IN_PLACE; tests/test_gpu_bases_in_place.py runs the same corpus on the device):
  * the shifted slicing, the sixteen-word identity test and the lazy negation, limb by limb against Python integers;
  * the affine start and the mixed addition on such bases at the value level: curve points against oracle/bn254_ref,
    coordinates at the edges of the range (p - 1, 1, all-ones words) against the formulas written out below;
  * tools/fq29_bounds.py with the scaled entries, and the zero-filter constants of the source against the bounds the
    tool derives (parsed from its output)."""
import os
import random
import re
import subprocess
import sys

import pytest

from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = o.P
MASK = (1 << 29) - 1
IN_W, OUT_W = 36, 40
OP = 40


def unpack_values():
    """Canonical E < p: the ends of the range, 2^253, the largest all-ones value below p, 2^254 - 1 reduced, alternating
    bits, all-ones in each single source word (the top word cut to stay below p)."""
    vs = [0, 1, 2, P - 1, P - 2, 1 << 253, (1 << 253) - 1, ((1 << 254) - 1) % P, int("55" * 32, 16) >> 2, int("AA" * 32, 16) >> 2]
    vs += [0xFFFFFFFF << (32 * w) for w in range(7)] + [0x2FFFFFFF << 224, (P >> 224) << 224]
    vs += [(1 << (29 * i - 3)) for i in range(1, 9)] + [(1 << (29 * i - 2)) - 1 for i in range(1, 9)]   # limb boundaries
    rng = random.Random(11)
    vs += [rng.randrange(P) for _ in range(32)]
    assert all(0 <= v < P for v in vs)
    return vs


def words8(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def record(recs, flags=0, mode=0):
    """(a, b) operand words of one element: up to three external (x, y) records, negate flags, mode."""
    recs = list(recs) + [(0, 0)] * (3 - len(recs))
    a = words8(recs[0][0]) + words8(recs[0][1]) + words8(recs[1][0]) + words8(recs[1][1]) + [flags] + [0] * 3
    b = [mode] + words8(recs[2][0]) + words8(recs[2][1]) + [0] * 19
    assert len(a) == IN_W and len(b) == IN_W
    return a, b


def run(op_fn, elems):
    a, b = [], []
    for ea, eb in elems:
        a += ea
        b += eb
    out = list(op_fn(OP, a, b, len(elems)))
    return [out[OUT_W * i:OUT_W * (i + 1)] for i in range(len(elems))]


def val(limbs):
    return sum(l << (29 * i) for i, l in enumerate(limbs))


def check_unpack(op_fn):
    vs = unpack_values()
    pairs = [(vs[i], vs[(i * 7 + 3) % len(vs)]) for i in range(len(vs))] + [(0, 0), (0, 1), (1, 0), (0, 1 << 255 >> 2)]
    outs = run(op_fn, [record([pr]) for pr in pairs])
    for (ex, ey), r in zip(pairs, outs):
        lx, ly, ny = r[0:9], r[9:18], r[19:28]
        assert all(l <= MASK for l in lx[:8] + ly[:8]), (hex(ex), hex(ey))
        assert val(lx) == ex << 3 and val(ly) == ey << 2, (hex(ex), hex(ey))
        assert r[18] == (1 if ex == 0 and ey == 0 else 0)
        assert all(0 <= l < 1 << 32 for l in ny) and val(ny) == 8 * P - (ey << 2), hex(ey)
        assert max(ny[:8]) < (1 << 30) + (1 << 29)   # limbs of the lazy negation: below 2^30.6, one operand of a product


def true_affine(pt_words):
    """XYZZ limbs (values V standing for V / rho) -> the affine point they denote on E', or None for ZZ = 0."""
    X, Y, ZZ, ZZZ = (val(pt_words[9 * k:9 * k + 9]) % P for k in range(4))
    if ZZ == 0:
        return None
    assert pow(ZZ, 3, P) == ZZZ * ZZZ * pow(2, 261, P) % P, "ZZ^3 = ZZZ^2 (in the internal domain: one rho apart)"
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def iso(pt):
    """E -> E': (x, y) -> (x / 4, y / 8)"""
    return None if pt is None else (pt[0] * pow(4, -1, P) % P, pt[1] * pow(8, -1, P) % P)


def ext(pt):
    return o.fq_to_mont(pt[0]), o.fq_to_mont(pt[1])


def formula_sum(pts):
    """madd-2008-s on field values, no curve needed: (p0 + p1) by the affine start, then + p2 by the mixed addition."""
    (x1, y1), (x2, y2) = pts[0], pts[1]
    Pd, R = (x2 - x1) % P, (y2 - y1) % P
    PP = Pd * Pd % P
    PPP = Pd * PP % P
    Q = x1 * PP % P
    X = (R * R - PPP - 2 * Q) % P
    Y = (R * (Q - X) - y1 * PPP) % P
    ZZ, ZZZ = PP, PPP
    if len(pts) == 3:
        x2, y2 = pts[2]
        Pd, R = (x2 * ZZ - X) % P, (y2 * ZZZ - Y) % P
        PP = Pd * Pd % P
        PPP = Pd * PP % P
        Q = X * PP % P
        X3 = (R * R - PPP - 2 * Q) % P
        Y = (R * (Q - X3) - Y * PPP) % P
        X, ZZ, ZZZ = X3, ZZ * PP % P, ZZZ * PPP % P
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def check_additions(op_fn):
    rng = random.Random(5)
    elems, want = [], []
    # curve points against the reference group law, every sign pattern, both modes
    G = [o.scalar_mul(rng.randrange(1, o.R_ORDER), o.GEN) for _ in range(6)]
    for flags in range(8):
        A, B, C = G[flags % 6], G[(flags + 1) % 6], G[(flags + 2) % 6]
        sg = [o.aff_neg(q) if (flags >> k) & 1 else q for k, q in enumerate((A, B, C))]
        elems.append(record([ext(A), ext(B)], flags, 1))
        want.append((iso(o.aff_add(sg[0], sg[1])), 0))
        elems.append(record([ext(A), ext(B), ext(C)], flags, 2))
        want.append((iso(o.aff_add(o.aff_add(sg[0], sg[1]), sg[2])), 0))
    A, B = G[0], G[1]
    elems.append(record([ext(A), ext(A)], 0, 1))           # doubling in the affine start
    want.append((iso(o.aff_add(A, A)), 0))
    elems.append(record([ext(A), ext(A)], 3, 1))           # ... of a negated base
    want.append((iso(o.aff_neg(o.aff_add(A, A))), 0))
    elems.append(record([ext(A), ext(A)], 2, 1))           # A + (-A): vanished
    want.append((None, 1))
    S = o.aff_add(A, B)
    elems.append(record([ext(A), ext(B), ext(S)], 0, 2))   # doubling in the mixed addition
    want.append((iso(o.aff_add(S, S)), 0))
    elems.append(record([ext(A), ext(B), ext(S)], 4, 2))   # (A + B) - (A + B): vanished
    want.append((None, 1))
    outs = run(op_fn, elems)
    for i, (r, (pt, vanished)) in enumerate(zip(outs, want)):
        assert r[36] == vanished, i
        if not vanished:
            assert true_affine(r) == pt, f"curve case {i}"
    # coordinates at the edges of the range (not curve points): the formulas on values
    edge = [P - 1, P - 2, 1, 2, (1 << 253) - 1, 1 << 253, 0xFFFFFFFF << 96, (P >> 224) << 224]
    elems, want = [], []
    for i in range(len(edge)):
        for flags in (0, 1, 2, 5, 7):
            e = [(edge[i], edge[(i + 3) % 8]), (edge[(i + 1) % 8], edge[(i + 5) % 8]), (edge[(i + 2) % 8], edge[(i + 6) % 8])]
            rinv = pow(2, 261, P)
            tv = []
            for k, (ex, ey) in enumerate(e):
                x, y = (ex << 3) * pow(rinv, -1, P) % P, (ey << 2) * pow(rinv, -1, P) % P
                tv.append((x, (-y) % P if (flags >> k) & 1 else y))
            for mode in (1, 2):
                elems.append(record(e, flags, mode))
                want.append(formula_sum(tv[:mode + 1]))
    outs = run(op_fn, elems)
    for i, (r, pt) in enumerate(zip(outs, want)):
        assert r[36] == 0 and true_affine(r) == pt, f"edge case {i}"
        for k in range(4):   # a returned point: limbs 0..7 normalised
            assert max(r[9 * k:9 * k + 8]) <= MASK + 8


def test_shifted_unpack_identity_and_negation_host(msm_pkg):
    check_unpack(msm_pkg.test_op_raw_host)


def test_affine_start_and_mixed_addition_on_the_isomorphic_curve_host(msm_pkg):
    check_additions(msm_pkg.test_op_raw_host)


def test_the_map_is_an_isomorphism_with_python_integers():
    """(x, y) -> (x / 4, y / 8) carries E onto y^2 = x^3 + 3/64, sums onto sums (a doubling included), and halving Z of
    a Jacobian point of E' gives the point of E."""
    rng = random.Random(2)
    A = o.scalar_mul(rng.randrange(1, o.R_ORDER), o.GEN)
    B = o.scalar_mul(rng.randrange(1, o.R_ORDER), o.GEN)
    b2 = 3 * pow(64, -1, P) % P
    for pt in (A, B, o.aff_add(A, B), o.aff_add(A, A)):
        x, y = iso(pt)
        assert (y * y - x * x * x - b2) % P == 0
    assert formula_sum([iso(A), iso(B)]) == iso(o.aff_add(A, B))
    assert formula_sum([iso(A), iso(B), iso(A)]) == iso(o.aff_add(o.aff_add(A, B), A))
    x, y = iso(A)
    z = rng.randrange(1, P)
    X, Y, Z = x * z * z % P, y * z * z * z % P, z * pow(2, -1, P) % P
    assert o.to_affine((X, Y, Z)) == A
    assert pow(3, (P - 1) // 2, P) == P - 1 and o.R_ORDER % 2 == 1   # no base has x = 0 or y = 0: (0, 0) marks the identity


def _tool():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fq29_bounds.py"), "-v"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_bounds_tool_passes_with_the_scaled_entries():
    out = _tool()
    for entry in ("pti_madd (E')", "pti_mmadd (E')", "pti_add_nz (E')", "pti_madd:", "pti_mmadd:", "pti_add_nz:"):
        assert entry in out, entry


def test_zero_filter_bounds_in_the_source_are_the_ones_the_tool_derives():
    derived = {m.group(1): (int(m.group(2)), int(m.group(3)))
               for m in re.finditer(r"zero filter (\w+): needs (\d+), the header has (\d+)", _tool())}
    src = open(os.path.join(ROOT, "metal-msm-gpu-acceleration_amd", "csrc", "bn254_ec29.hip.h")).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (kZeroFilter\w+) = (\d+);", src)}
    assert set(derived) == set(consts) == {"kZeroFilterMadd", "kZeroFilterMmadd", "kZeroFilterMmaddIso", "kZeroFilterAdd"}
    for name, (needs, has) in derived.items():
        assert needs == has == consts[name], name
    # every filter of the shipped additions takes its bound from these constants
    shipped = src.split("#if defined(MSM_AMD_EXPERIMENTS) && (defined(MSM_FQ29_LOCKSTEP)")[0] + src.split("// p + q, BOTH affine")[1]
    uses = re.findall(r"maybe_zero\(\w+, ([^)]*)\)", shipped)
    assert sorted(uses) == sorted(["kZeroFilterMadd", "ISO ? kZeroFilterMmaddIso : kZeroFilterMmadd", "kZeroFilterAdd"]), uses
    assert consts["kZeroFilterMmaddIso"] > consts["kZeroFilterMmadd"]   # the bound of E would miss equal-x pairs on E'
