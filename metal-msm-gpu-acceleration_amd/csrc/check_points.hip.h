// Point validation (msm_amd_check_points*, msm_amd_g2_check_points* and their host twins): the per-record bodies that
// k_check.hip runs one lane per record and host_check.hip runs on the CPU.  A record gets ONE reason code, the first
// rule that fails:
//   1 NOT_REDUCED       some coordinate, read as a 256-bit integer in the layout's own form, is >= p
//   2 NOT_ON_CURVE      G1: y^2 != x^3 + 3 (Jacobian: Y^2 != X^3 + 3 Z^6);  G2: y^2 != x^3 + 3 / (9 + u)
//   3 NOT_IN_SUBGROUP   G2 only: on the curve, but [r] P != O
// Identity encodings are valid: (0, 0) of the halo2curves layouts, the flag of the ark affine layouts (whatever the
// coordinate bytes, the rule of load_ext_g2 / ark_affine_to_affine_kernel), Z = 0 of the G1 Jacobian layouts (whose
// coordinates are still range-checked).
//
// Curve equation.  The coordinates go through Fq29::from_ext (outputs < 1.01 p); t = x^2 x < 1.01 p (Fq2: x^2 < 1.4 p,
// x^2 x < 1.20 p); the subtrahend t + b < 4.2 p (b = 3 rho < p, Jacobian 3 Z^6 < 3.1 p) goes through the 8 p lift and
// the difference y^2 - t - b + 8 p < 9.4 p is decided by is_zero_exact (one squash and a canonical compare), never by
// the one-limb filter alone.
//
// G2 subgroup rule.  [r] P = O is decided by the endomorphism identity of BN curves with parameter x0 (M. Scott,
// "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly curves", 2021, section on BN curves):
//     [x0 + 1] P + psi([x0] P) + psi^2([x0] P) = psi^3([2 x0] P)       x0 = 4965661367192848881
// with psi(x, y) = (conj(x) gx, conj(y) gy), gx = xi^((p - 1) / 3), gy = xi^((p - 1) / 2), xi = 9 + u, the
// untwist-Frobenius-twist map.  Evaluated as  D = P + Q + psi(Q + psi(Q - psi(2 Q))),  Q = [x0] P, and D == O: one
// 63-bit double-and-add, three psi, one doubling, four additions -- about a quarter of the plain 254-bit ladder.
// Every step uses the additions with their exceptional branches (P + P, P + (-P), identity operands): the twist has
// points of small order (10069 divides the cofactor 2 p - r) and the ladder meets them.  The cofactor is odd, so no
// point of the curve has y = 0 and pt2_double never sees one.
//
// Bounds (multiples of p per component, the XYZZ invariant X < 1.21, Y < 13.4, ZZ < 3.2, ZZZ < 2.04 of
// bn254_ec2_29.hip.h; tools/g2_bounds.py re-derives them):
//   conj(a) negates c1 through a lift: 32 p - c1 for X, Y (then the SECOND operand of Fq2::mul, whose b1 may be
//   anything < 32 p), 4 p - c1 for ZZ, ZZZ (< 4 p: both are < 3.2 p)
//   psi: X' = gx conj(X): c0 < 1 + rho'(1 * 1.21 + 32 * 1) = 1.20, c1 < 1 + rho'(1 * 32 + 1 * 1.21) = 1.20  (< 1.21)
//        Y' = gy conj(Y): < 1 + rho'(13.4 + 32) = 1.27                                                  (< 13.4)
//        ZZ' = squash(conj(ZZ)), ZZZ' = squash(conj(ZZZ)): < 1 + rho' 4 = 1.03                           (< 3.2, 2.04)
//   -R:  Y' = squash(32 p - Y) < 1 + rho' 32 = 1.19                                                     (< 13.4)
//   final comparison: D = L + (-R) by pt2_add; D == O iff the addition vanished or both operands were the identity --
//   pt2_add_nz returns exact zero limbs then, and a finite sum has ZZ = ZZ1 ZZ2 PP != 0 mod p (P was tested exactly).
#pragma once
#include <string.h>

#include "bn254_ec2_29.hip.h"
#include "point_report.hip.h"

namespace msm_amd {

enum : uint32_t { kCheckCurve = 1, kCheckSubgroup = 2 };
// Point layouts as the C ABI numbers them (MSM_AMD_POINT_*, MSM_AMD_G2_POINT_*; host_check.hip asserts the match)
enum : int { kLayoutH2cAffine = 0, kLayoutArkProjective = 1, kLayoutArkAffine = 2, kLayoutJacBe32 = 3, kLayoutPrepared = 4 };
enum : int { kG2LayoutH2cAffine = 0, kG2LayoutArkAffine = 1, kG2LayoutPrepared = 2 };
// Kinds of layout an entry point may accept: the affine host layouts, the Jacobian / projective host layouts (G1 only),
// the library's own *_PREPARED records
enum : uint32_t { kKindAffine = 1, kKindJacobian = 2, kKindPrepared = 4, kKindHost = kKindAffine | kKindJacobian };

// Record size of `layout` in its group if the layout is of one of `kinds`, 0 otherwise (unknown layouts, *_TABLES)
MSM_HD uint32_t point_record_bytes(bool g2, int layout, uint32_t kinds) {
  uint32_t kind = 0, bytes = 0;
  if (g2) {
    if (layout == kG2LayoutH2cAffine) kind = kKindAffine, bytes = 128;
    else if (layout == kG2LayoutArkAffine) kind = kKindAffine, bytes = 136;
    else if (layout == kG2LayoutPrepared) kind = kKindPrepared, bytes = 128;
  } else {
    if (layout == kLayoutH2cAffine) kind = kKindAffine, bytes = 64;
    else if (layout == kLayoutArkAffine) kind = kKindAffine, bytes = 72;
    else if (layout == kLayoutArkProjective || layout == kLayoutJacBe32) kind = kKindJacobian, bytes = 96;
    else if (layout == kLayoutPrepared) kind = kKindPrepared, bytes = 64;
  }
  return (kind & kinds) ? bytes : 0u;
}

constexpr uint64_t kBnX0 = 4965661367192848881ull;   // p = 36 x0^4 + 36 x0^3 + 24 x0^2 + 6 x0 + 1, 63 bits

// Word `w` of a record (records of the ark affine layouts are only 8-byte aligned: word loads throughout)
MSM_HD uint32_t check_word(const uint8_t* rec, int w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return reinterpret_cast<const uint32_t*>(rec)[w];
#else
  uint32_t v;
  memcpy(&v, rec + 4 * w, 4);
  return v;
#endif
}
// 256-bit value at word `off`; be32: most significant word first (the reference wire layout)
MSM_HD u256 check_u256(const uint8_t* rec, int off, bool be32 = false) {
  u256 r;
  MSM_UNROLL for (int i = 0; i < 8; ++i) r.v[i] = check_word(rec, off + (be32 ? 7 - i : i));
  return r;
}
MSM_HD bool check_ge_p(const u256& a) {
  u256 d;
  return u256_sub(d, a, Fq::modulus()) == 0;
}

// ---- G1 ----------------------------------------------------------------------------------------------------------
MSM_HD fe29 check_b_g1() {   // 3 rho mod p
  constexpr uint32_t c[9] = {0x00766463u, 0x1C54760Au, 0x08F6927Au, 0x03E40C4Du, 0x1FEA4F2Bu,
                             0x17C6C26Au, 0x157FE417u, 0x0F8056F9u, 0x002958A2u};
  fe29 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) r.l[i] = c[i];
  return r;
}

// y^2 == x^3 + b with b given (b < 3.1 p)
MSM_HD bool check_curve_g1(const fe29& x, const fe29& y, const fe29& b) {
  const fe29 t = Fq29::mul(Fq29::sqr(x), x);
  const fe29 d = Fq29::norm(Fq29::sub<K8E30>(Fq29::sqr(y), Fq29::norm(Fq29::add(t, b))));
  return Fq29::is_zero_exact(d);
}

// One G1 record in the caller's layout -> reason code; `identity`: valid as an identity encoding.
MSM_HD uint32_t check_record_g1(int layout, const uint8_t* rec, bool& identity) {
  identity = false;
  if (layout == kLayoutArkAffine && (check_word(rec, 16) & 0xFFu)) {
    identity = true;
    return kPointValid;
  }
  const bool jac = layout == kLayoutArkProjective || layout == kLayoutJacBe32;
  const bool be = layout == kLayoutJacBe32;
  const u256 x = check_u256(rec, 0, be), y = check_u256(rec, 8, be);
  const u256 z = jac ? check_u256(rec, 16, be) : u256_zero();
  if (check_ge_p(x) || check_ge_p(y) || (jac && check_ge_p(z))) return kPointNotReduced;
  if (jac ? u256_is_zero(z) : (layout == kLayoutH2cAffine && u256_is_zero(x) && u256_is_zero(y))) {
    identity = true;
    return kPointValid;
  }
  fe29 b = check_b_g1();
  if (jac) {   // 3 Z^6
    const fe29 z1 = Fq29::from_ext(z);
    const fe29 z2 = Fq29::sqr(z1);
    const fe29 z6 = Fq29::mul(Fq29::sqr(z2), z2);
    b = Fq29::norm(Fq29::add(z6, Fq29::add(z6, z6)));
  }
  return check_curve_g1(Fq29::from_ext(x), Fq29::from_ext(y), b) ? kPointValid : kPointNotOnCurve;
}

// ---- G2 ----------------------------------------------------------------------------------------------------------
// Constants of the internal domain (value * 2^261 mod p, 29-bit limbs).  b' = 3 / (9 + u) = 3 (9 - u) / 82:
//   b'.c0 = 27 / 82 = 19485874751759354771024239261021720505790618469301721065564631296452457478373
//   b'.c1 = -3 / 82 =   266929791119991161246907387137283842545076965332900288569378510910307636690
// (tests/test_check_host.py pins the limbs against tests/g2_ref.py::B_TWIST and gx, gy against xi^((p-1)/3), xi^((p-1)/2))
MSM_HD constexpr uint32_t check_g2_const(int which, int i) {
  constexpr uint32_t c[6][9] = {
      // b'.c0, b'.c1
      {0x0B489658u, 0x00CFD255u, 0x0FDB9A77u, 0x02CE89F7u, 0x0033A0D4u, 0x1A768545u, 0x06EE3DDCu, 0x106A7DC1u, 0x0019316Bu},
      {0x1B9FECE0u, 0x07ECCCD1u, 0x1069F1C7u, 0x0CDF64F3u, 0x0154CBE1u, 0x0DD22AC0u, 0x06EBA4E8u, 0x1929A235u, 0x00283739u},
      // gx = xi^((p - 1) / 3)
      {0x04A59190u, 0x06F504D9u, 0x0BF870BBu, 0x171FFD5Cu, 0x1AC4D17Du, 0x04BE36D5u, 0x0BCEEC27u, 0x1A83A513u, 0x002492B3u},
      {0x11142EF1u, 0x0B31ACC7u, 0x1D5818BCu, 0x180AFC17u, 0x1A63177Eu, 0x15765B3Bu, 0x118F742Eu, 0x063A509Au, 0x00135E4Eu},
      // gy = xi^((p - 1) / 2)
      {0x1B1F0678u, 0x0373FB06u, 0x13170FBDu, 0x185D74B7u, 0x0241131Fu, 0x16E18435u, 0x1EF3B6CEu, 0x01F06F02u, 0x001D46BDu},
      {0x19A647D5u, 0x19FDEFABu, 0x1D925D1Au, 0x0D1F6C5Fu, 0x08AC6CC5u, 0x1FA5621Au, 0x134F06FEu, 0x09A72816u, 0x0015871Du}};
  return c[which][i];
}
MSM_HD fq2 check_g2_fq2(int which) {   // 0: b', 1: gx, 2: gy
  fq2 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) {
    r.c0.l[i] = check_g2_const(2 * which, i);
    r.c1.l[i] = check_g2_const(2 * which + 1, i);
  }
  return r;
}

MSM_HD bool check_curve_g2(const Aff2I& a) {
  const fq2 t = Fq2::mul(Fq2::sqr(a.x), a.x);
  const fq2 d = Fq2::sub<8>(Fq2::sqr(a.y), Fq2::norm(Fq2::add(t, check_g2_fq2(0))));
  return Fq2::is_zero_exact(d);
}

// psi on an XYZZ point (identity -> identity): no inversion, see the bounds in the header comment
MSM_HD PtI2 pt2_psi(const PtI2& p) {
  if (pt2_is_identity(p)) return p;
  PtI2 r;
  r.x = Fq2::mul(check_g2_fq2(1), fq2{p.x.c0, Fq2::sub1<32>(Fq29::zero(), p.x.c1)});
  r.y = Fq2::mul(check_g2_fq2(2), fq2{p.y.c0, Fq2::sub1<32>(Fq29::zero(), p.y.c1)});
  r.zz = Fq2::squash(fq2{p.zz.c0, Fq2::sub1<4>(Fq29::zero(), p.zz.c1)});
  r.zzz = Fq2::squash(fq2{p.zzz.c0, Fq2::sub1<4>(Fq29::zero(), p.zzz.c1)});
  return r;
}
MSM_HD PtI2 pt2_neg(const PtI2& p) {
  if (pt2_is_identity(p)) return p;
  PtI2 r = p;
  r.y = Fq2::squash(Fq2::neg(p.y));
  return r;
}
MSM_HD PtI2 pt2_double_any(const PtI2& p) { return pt2_is_identity(p) ? p : pt2_double(p); }
// acc + q, acc any XYZZ point, q affine and finite
MSM_HD PtI2 pt2_madd_any(const PtI2& acc, const Aff2I& q) {
  if (pt2_is_identity(acc)) return pt2_from_aff(q);
  bool vanished = false;
  return pt2_madd(acc, q, vanished);
}

// [r] P == O for a finite point P of the curve (internal affine form, from_ext outputs).  The ladder's base is
// canonicalised first, as the stored bases of the MSM are: the XYZZ invariant is derived for canonical bases.
MSM_HD bool check_subgroup_g2(const Aff2I& p) {
  Aff2I a;
  a.x = fq2{Fq29::canonical(p.x.c0, 1), Fq29::canonical(p.x.c1, 1)};
  a.y = fq2{Fq29::canonical(p.y.c0, 1), Fq29::canonical(p.y.c1, 1)};
  PtI2 q = pt2_from_aff(a);   // bit 62 of x0
  MSM_NO_UNROLL for (int b = 61; b >= 0; --b) {
    q = pt2_double_any(q);
    if ((kBnX0 >> b) & 1ull) q = pt2_madd_any(q, a);
  }
  PtI2 d = pt2_add(q, pt2_neg(pt2_psi(pt2_double_any(q))));   // Q - psi(2 Q)
  d = pt2_add(q, pt2_psi(d));                                 // Q + psi(Q - psi(2 Q))
  d = pt2_add(q, pt2_psi(d));                                 // Q + psi(Q + psi(Q - psi(2 Q)))
  d = pt2_madd_any(d, a);                                     // ... + P
  return pt2_is_identity(d);
}

// One G2 record (ark != 0: 136-byte records with the infinity flag at byte 128) -> reason code
MSM_HD uint32_t check_record_g2(int ark, const uint8_t* rec, uint32_t checks, bool& identity) {
  identity = false;
  if (ark && (check_word(rec, 32) & 0xFFu)) {
    identity = true;
    return kPointValid;
  }
  Affine2 e;
  e.x.c0 = check_u256(rec, 0);
  e.x.c1 = check_u256(rec, 8);
  e.y.c0 = check_u256(rec, 16);
  e.y.c1 = check_u256(rec, 24);
  if (check_ge_p(e.x.c0) || check_ge_p(e.x.c1) || check_ge_p(e.y.c0) || check_ge_p(e.y.c1)) return kPointNotReduced;
  if (!ark && affine2_is_identity(e)) {
    identity = true;
    return kPointValid;
  }
  Aff2I a;
  a.x = Fq2::from_ext(e.x.c0, e.x.c1);
  a.y = Fq2::from_ext(e.y.c0, e.y.c1);
  if (!check_curve_g2(a)) return kPointNotOnCurve;
  if ((checks & kCheckSubgroup) && !check_subgroup_g2(a)) return kPointNotInSubgroup;
  return kPointValid;
}

}  // namespace msm_amd
