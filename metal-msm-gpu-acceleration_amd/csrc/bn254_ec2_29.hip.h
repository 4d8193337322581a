// BN254 G2 group law on Fq2 = Fq[u] / (u^2 + 1) (bn254_fq2_29.hip.h): the arithmetic of the G2 kernels (k_g2.hip).
// The curve is the sextic twist y^2 = x^3 + b' with b' = 3 / (9 + u); no formula below uses b' (a = 0 short
// Weierstrass formulas need only a), so only the host and test code carry the constant.  Points in HBM:
//   Aff2Packed 128 bytes: canonical x.c0, x.c1, y.c0, y.c1 of the internal Montgomery domain, 32 bytes each (the G1
//              AffPacked layout twice); the identity is x.c0 = 2^256 - 1, the marker of AffPacked
//   PtI2       288 bytes: X, Y, ZZ, ZZZ in Fq2 (4 x 2 x 9 limbs), extended Jacobian "XYZZ" as in bn254_ec29.hip.h;
//              ZZ limbs all zero = identity
// Formulas (EFD, XYZZ, a = 0), the ones of G1: mixed addition madd-2008-s, its affine + affine start mmadd-2008-s,
// full addition add-2008-s, doubling dbl-2008-s-1, each product an Fq2 product.  X3 is squashed (one multiplication
// by rho mod p per component) before it is stored: the lazily reduced X then stays below 1.21 p and the subtraction
// U2 - X1 of the next addition needs only 4 p of lift.  Value bounds of every stored or carried point (multiples of p,
// per component; tools/g2_bounds.py):
//      X < 1.21 p     Y < 13.4 p     ZZ < 3.2 p     ZZZ < 2.04 p     all components normalised
// Intermediate values stay below 20 p (P < 9.3 p, R < 20 p), inside the 32 p lift of Fq2::mul / sqr.  The
// exceptional cases (P = Q -> doubling, P = -Q -> identity) are filtered on the one-limb test of both components of P
// (Fq2::maybe_zero, bound 16 > 9.3) and confirmed exactly; the doubling squashes all of its outputs.
// XYZZ -> affine (pt2_to_affine, the table build) costs ONE inversion: t = (ZZ ZZZ)^-1, x = X t ZZZ, y = Y t ZZ.
// For any carried point (bounds above): ZZ ZZZ < 1.7 p, t < 1.2 p, X t < 1.24 p, Y t < 3.7 p, x < 1.25 p,
// y < 1.3 p -- multiplication outputs below 2 p, what aff2_pack takes.
#pragma once
#include "bn254_ec.hip.h"
#include "bn254_fq2_29.hip.h"

namespace msm_amd {

// external forms: halo2curves bn256::G2Affine (128 B) and the 192-byte Jacobian result, Montgomery R = 2^256
struct Fq2Ext {
  u256 c0, c1;
};
struct Affine2 {
  Fq2Ext x, y;
};
struct Jacobian2 {
  Fq2Ext x, y, z;
};
struct Aff2I {   // register form of a base
  fq2 x, y;
};
struct Aff2Packed {   // memory form: canonical internal x.c0, x.c1, y.c0, y.c1
  u256 x0, x1, y0, y1;
};
struct PtI2 {
  fq2 x, y, zz, zzz;
};
static_assert(sizeof(Affine2) == 128, "Affine2 must be 128 bytes");
static_assert(sizeof(Jacobian2) == 192, "Jacobian2 must be 192 bytes");
static_assert(sizeof(Aff2Packed) == 128, "Aff2Packed must be 128 bytes");
static_assert(sizeof(PtI2) == 288, "PtI2 must be 288 bytes");

constexpr uint32_t kG2ZeroFilter = 16;   // one-limb zero filter bound: every tested P < 9.3 p

MSM_HD bool affine2_is_identity(const Affine2& p) {
  return u256_is_zero(p.x.c0) && u256_is_zero(p.x.c1) && u256_is_zero(p.y.c0) && u256_is_zero(p.y.c1);
}
MSM_HD bool aff2i_is_identity(const Aff2I& p) { return Fq2::is_zero_limbs(p.x) && Fq2::is_zero_limbs(p.y); }
MSM_HD bool pt2_is_identity(const PtI2& p) { return Fq2::is_zero_limbs(p.zz); }

MSM_HD PtI2 pt2_identity() {
  PtI2 r;
  r.x = Fq2::one();
  r.y = Fq2::one();
  r.zz = Fq2::zero();
  r.zzz = Fq2::zero();
  return r;
}

MSM_HD PtI2 pt2_from_aff(const Aff2I& q) {   // q not the identity; q.y may be a negation (< 4 p)
  PtI2 r;
  r.x = q.x;
  r.y = q.y;
  r.zz = Fq2::one();
  r.zzz = Fq2::one();
  return r;
}

// ---- conversions ---------------------------------------------------------------------------------------
MSM_HD Aff2I aff2i_from_ext(const Affine2& p) {   // the identity (all zero) -> exact zero limbs
  Aff2I r;
  if (affine2_is_identity(p)) {
    r.x = Fq2::zero();
    r.y = Fq2::zero();
  } else {
    r.x = Fq2::from_ext(p.x.c0, p.x.c1);
    r.y = Fq2::from_ext(p.y.c0, p.y.c1);
  }
  return r;
}
MSM_HD Aff2Packed aff2_pack(const Aff2I& p) {   // p from aff2i_from_ext (multiplication outputs or exact zeros)
  Aff2Packed r;
  r.x0 = Fq29::pack_canonical(p.x.c0);   // the identity's zero limbs pack to zero ...
  r.x1 = Fq29::pack_canonical(p.x.c1);
  r.y0 = Fq29::pack_canonical(p.y.c0);
  r.y1 = Fq29::pack_canonical(p.y.c1);
  const uint32_t mark = aff2i_is_identity(p) ? 0xFFFFFFFFu : 0u;   // ... and gets its marker (a select, not a branch:
  MSM_UNROLL for (int i = 0; i < 8; ++i) r.x0.v[i] |= mark;         // the branch form put the record on the stack)
  return r;
}
MSM_HD bool aff2packed_is_identity(const Aff2Packed& p) { return p.x0.v[7] == 0xFFFFFFFFu; }
MSM_HD Aff2I aff2_unpack_finite(const Aff2Packed& p) {
  Aff2I r;
  r.x.c0 = Fq29::unpack256(p.x0);
  r.x.c1 = Fq29::unpack256(p.x1);
  r.y.c0 = Fq29::unpack256(p.y0);
  r.y.c1 = Fq29::unpack256(p.y1);
  return r;
}

// memory form -> external affine (canonical Montgomery R = 2^256; the identity marker -> all zero)
MSM_HD Affine2 aff2packed_to_ext(const Aff2Packed& p) {
  Affine2 r;
  if (aff2packed_is_identity(p)) {
    r.x.c0 = r.x.c1 = r.y.c0 = r.y.c1 = u256_zero();
    return r;
  }
  const Aff2I a = aff2_unpack_finite(p);
  Fq2::to_ext(a.x, r.x.c0, r.x.c1);
  Fq2::to_ext(a.y, r.y.c0, r.y.c1);
  return r;
}

// Jacobian (X, Y, Z) -> (X, Y, Z^2, Z^3)
MSM_HD PtI2 pt2_from_ext(const Jacobian2& p) {
  if (u256_is_zero(p.z.c0) && u256_is_zero(p.z.c1)) return pt2_identity();
  PtI2 r;
  r.x = Fq2::squash(Fq2::from_ext(p.x.c0, p.x.c1));
  r.y = Fq2::from_ext(p.y.c0, p.y.c1);
  const fq2 z = Fq2::from_ext(p.z.c0, p.z.c1);
  r.zz = Fq2::sqr(z);
  r.zzz = Fq2::mul(r.zz, z);
  return r;
}
// (X, Y, ZZ, ZZZ) -> Jacobian (X ZZ, Y ZZZ, ZZ); the identity -> (1, 1, 0) in Montgomery form
MSM_HD Jacobian2 pt2_to_ext(const PtI2& p) {
  Jacobian2 r;
  if (pt2_is_identity(p)) {
    r.x.c0 = Fq::one();
    r.x.c1 = u256_zero();
    r.y = r.x;
    r.z.c0 = u256_zero();
    r.z.c1 = u256_zero();
    return r;
  }
  Fq2::to_ext(Fq2::mul(p.x, p.zz), r.x.c0, r.x.c1);
  Fq2::to_ext(Fq2::mul(p.y, p.zzz), r.y.c0, r.y.c1);
  Fq2::to_ext(p.zz, r.z.c0, r.z.c1);
  return r;
}

// ---- rare path: doubling (an addition of two equal points) ---------------------------------------------
// dbl-2008-s-1 (a = 0): 6M + 3S; the outputs are squashed (the path is rare, its bounds then need no care).
MSM_HD PtI2 pt2_double(const PtI2& p) {   // p not the identity
  const fq2 U = Fq2::norm(Fq2::add(p.y, p.y));                              // < 26.8 p
  const fq2 V = Fq2::sqr(U);
  const fq2 W = Fq2::mul(U, V);
  const fq2 S = Fq2::mul(p.x, V);
  const fq2 XX = Fq2::sqr(p.x);
  const fq2 M = Fq2::norm(Fq2::add(XX, Fq2::add(XX, XX)));
  PtI2 r;
  r.x = Fq2::squash(Fq2::sub<32>(Fq2::sqr(M), Fq2::norm(Fq2::add(S, S))));   // M^2 - 2S
  const fq2 T = Fq2::sub<4>(S, r.x);                                           // S - X3
  r.y = Fq2::squash(Fq2::sub<8>(Fq2::mul(M, T), Fq2::mul(W, p.y)));          // M (S - X3) - W Y1
  r.zz = Fq2::squash(Fq2::mul(V, p.zz));
  r.zzz = Fq2::squash(Fq2::mul(W, p.zzz));
  return r;
}

// (X, Y, ZZ, ZZZ), not the identity -> affine (X / ZZ, Y / ZZZ) with one inversion.  The outputs are multiplication
// results below 2 p (header), NOT canonical: aff2_pack canonicalises them.
MSM_HD Aff2I pt2_to_affine(const PtI2& p) {
  const fq2 t = Fq2::inv(Fq2::mul(p.zz, p.zzz));
  Aff2I r;
  r.x = Fq2::mul(Fq2::mul(p.x, t), p.zzz);
  r.y = Fq2::mul(Fq2::mul(p.y, t), p.zz);
  return r;
}

// The precomputed window tables of one base (build_tables_g2_kernel and its host twin): entry w = 2^(c w) P as
// Aff2Packed, handed to put(w, record).  Window 0 is the converted base; window w is c doublings of window w - 1,
// re-started from its stored affine entry (canonical coordinates, ZZ = ZZZ = 1), then pt2_to_affine.  P is taken as a
// point of odd order (r-torsion), so no doubling meets y = 0; the identity stays the identity marker throughout.
template <class Put>
MSM_HD void g2_table_walk(const Affine2& ext, uint32_t c, uint32_t W, Put&& put) {
  Aff2Packed rec = aff2_pack(aff2i_from_ext(ext));
  put(0u, rec);
  const bool ident = aff2packed_is_identity(rec);
  MSM_NO_UNROLL for (uint32_t w = 1; w < W; ++w) {
    if (!ident) {
      PtI2 p = pt2_from_aff(aff2_unpack_finite(rec));
      MSM_NO_UNROLL for (uint32_t i = 0; i < c; ++i) p = pt2_double(p);
      rec = aff2_pack(pt2_to_affine(p));
    }
    put(w, rec);
  }
}

// The common tail of the additions: X3 = R^2 - PPP - 2Q (squashed), Y3 = R (Q - X3) - S1 PPP.
MSM_HD void pt2_tail(const fq2& P, const fq2& R, const fq2& U1, const fq2& S1, PtI2& r, fq2& PP, fq2& PPP) {
  PP = Fq2::sqr(P);
  PPP = Fq2::mul(P, PP);
  const fq2 Q = Fq2::mul(U1, PP);
  const fq2 RR = Fq2::sqr(R);
  r.x = Fq2::squash(Fq2::sub<16>(RR, Fq2::norm(Fq2::add(PPP, Fq2::add(Q, Q)))));   // < 1.21 p
  const fq2 T = Fq2::sub<4>(Q, r.x);
  r.y = Fq2::sub<8>(Fq2::mul(R, T), Fq2::mul(S1, PPP));                          // < 13.4 p
}

// p + q, p XYZZ (not identity), q affine (not identity; q.y may be a negation < 4 p).  madd-2008-s.
// `reload_q` gives q again for the exceptional case q == p (the caller may have re-used its registers).
template <class ReloadQ>
MSM_HD PtI2 pt2_madd(const PtI2& p, const fq2& qx, const fq2& qy, ReloadQ&& reload_q, bool& vanished) {
  const fq2 U2 = Fq2::mul(qx, p.zz);
  const fq2 S2 = Fq2::mul(qy, p.zzz);
  const fq2 P = Fq2::sub<4>(U2, p.x);    // < 5.3 p
  const fq2 R = Fq2::sub<16>(S2, p.y);   // < 17.8 p
  if (Fq2::maybe_zero(P, kG2ZeroFilter)) {
    if (Fq2::is_zero_exact(P)) {   // same x: q == p (double) or q == -p (identity)
      if (Fq2::is_zero_exact(R)) return pt2_double(pt2_from_aff(reload_q()));
      vanished = true;
      return pt2_identity();
    }
  }
  PtI2 r;
  fq2 PP, PPP;
  pt2_tail(P, R, p.x, p.y, r, PP, PPP);
  r.zz = Fq2::mul(p.zz, PP);
  r.zzz = Fq2::mul(p.zzz, PPP);
  return r;
}

// p + q, BOTH affine and not the identity: madd with ZZ1 = ZZZ1 = 1 (mmadd-2008-s).  p.y, q.y may be negations.
template <class ReloadQ>
MSM_HD PtI2 pt2_mmadd(const fq2& px, const fq2& py, const fq2& qx, const fq2& qy, ReloadQ&& reload_q,
                      bool& vanished) {
  const fq2 P = Fq2::sub<4>(qx, px);
  const fq2 R = Fq2::sub<16>(qy, py);   // < 20 p
  if (Fq2::maybe_zero(P, kG2ZeroFilter)) {
    if (Fq2::is_zero_exact(P)) {
      if (Fq2::is_zero_exact(R)) return pt2_double(pt2_from_aff(reload_q()));
      vanished = true;
      return pt2_identity();
    }
  }
  PtI2 r;
  fq2 PP, PPP;
  pt2_tail(P, R, px, py, r, PP, PPP);
  r.zz = PP;
  r.zzz = PPP;
  return r;
}
MSM_HD PtI2 pt2_madd(const PtI2& p, const Aff2I& q, bool& vanished) {
  return pt2_madd(p, q.x, q.y, [&]() { return q; }, vanished);
}
MSM_HD PtI2 pt2_mmadd(const Aff2I& p, const Aff2I& q, bool& vanished) {
  return pt2_mmadd(p.x, p.y, q.x, q.y, [&]() { return q; }, vanished);
}

// p + q, both XYZZ, neither the identity: add-2008-s (12M + 2S).
MSM_HD PtI2 pt2_add_nz(const PtI2& p, const PtI2& q, bool& vanished) {
  const fq2 U1 = Fq2::mul(p.x, q.zz);
  const fq2 U2 = Fq2::mul(q.x, p.zz);
  const fq2 S1 = Fq2::mul(p.y, q.zzz);
  const fq2 S2 = Fq2::mul(q.y, p.zzz);
  const fq2 P = Fq2::sub<8>(U2, U1);   // < 9.3 p
  const fq2 R = Fq2::sub<8>(S2, S1);   // < 11.1 p
  if (Fq2::maybe_zero(P, kG2ZeroFilter)) {
    if (Fq2::is_zero_exact(P)) {
      if (Fq2::is_zero_exact(R)) return pt2_double(p);
      vanished = true;   // q == -p
      return pt2_identity();
    }
  }
  PtI2 r;
  fq2 PP, PPP;
  pt2_tail(P, R, U1, S1, r, PP, PPP);
  r.zz = Fq2::mul(Fq2::mul(p.zz, q.zz), PP);
  r.zzz = Fq2::mul(Fq2::mul(p.zzz, q.zzz), PPP);
  return r;
}
MSM_HD PtI2 pt2_add_nz(const PtI2& p, const PtI2& q) {
  bool vanished = false;
  return pt2_add_nz(p, q, vanished);
}
// General addition, identity operands allowed.
MSM_HD PtI2 pt2_add(const PtI2& p, const PtI2& q) {
  if (pt2_is_identity(p)) return q;
  if (pt2_is_identity(q)) return p;
  return pt2_add_nz(p, q);
}

}  // namespace msm_amd
