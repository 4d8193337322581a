// Batch scalar multiplication (msm_amd_mul_points*, msm_amd_g2_mul_points* and their host twins): out[i] = [s_i] P_i
// (kMulBaseEach) or out[i] = [s_i] P (kMulBaseOne), written as canonical affine records.  The per-record bodies that
// k_mul.hip runs one lane per record and host_mul.hip runs on the CPU.  Both groups share every body below through the
// traits MulG1 / MulG2 (point types, additions, field of the coordinates).
//
// Scalars: the three MSM_AMD_SCALAR_* layouts, reduced exactly as the MSM's digit code reduces them (mul_scalar: a
// Montgomery record leaves the domain, a canonical one is brought below r by at most five subtractions).  The result
// is [s] P for that INTEGER s < r: no step below uses the group order, so a G2 base outside the r-torsion is
// multiplied as a curve point.
//
// One base (kMulBaseOne).  mul_table_entry builds T[w][d - 1] = [d 2^(c w)] P for d = 1 .. 2^(c-1), c = kMulWindow = 8,
// w < kMulWindows = 32: 4096 packed affine entries (256 KiB for G1, 512 KiB for G2: L2-resident), one lane per entry, a
// ladder over the 256-bit integer d 2^(c w) and one inversion through the existing to-affine paths.  mul_fixed walks
// the signed digits of the scalar (the digit rule of scalar_digits in k_sort.hip: a window value above 2^(c-1) becomes
// v - 2^c with a carry into the next window; the top window takes the last carry, s < 2^254), skips zero digits, starts
// the accumulator at the first non-zero digit and adds every further table entry by a mixed addition: at most 32
// additions per output, no doubling.
// Base per scalar (kMulBaseEach).  mul_ladder: 256 doubling steps and one mixed addition per set bit on XYZZ with the
// affine base, the ladder of check_subgroup_g2.  Every step uses the additions with their exceptional branches: a G2
// base of order 10069 makes a partial sum equal to the base or to its negative.
// Either way the result stays XYZZ; mul_normalise turns kMulNormGroup = 16 consecutive XYZZ records into affine ones
// with ONE inversion (Montgomery's trick), in place in the record buffer:
//   forward, i = 0 .. m-1:  a_i = ZZ_i ZZZ_i,  record_i <- (X_i ZZZ_i, Y_i ZZ_i, a_i, pre_(i-1)),  pre_i = pre_(i-1) a_i
//   inv = 1 / pre_(m-1)
//   backward, i = m-1 .. 0: t_i = inv pre_(i-1) = 1 / a_i,  inv <- inv a_i,  x_i = (X_i ZZZ_i) t_i,  y_i = (Y_i ZZ_i) t_i
// An identity record takes a_i = 1 and numerators of exact zero limbs: the chain is not zeroed, x_i = y_i = exact zero
// limbs and the store writes the layout's identity encoding.  8 products per output and 370 / 16 = 23 for its share
// of the inversion.
//
// Bounds (multiples of p per component, rho' = p / rho = 0.0059; tools/fq29_bounds.py re-derives the G1 figures,
// tools/g2_bounds.py the G2 ones).
// G1, the invariant of bn254_ec29.hip.h (X < 10, Y < 6, ZZ < 2.8, ZZZ < 2):
//   base: from_ext output < 1.04, canonicalised.  negated entry: y' = 4 p - y, normalised (pti_madd: q.y < 4 p)
//   pti_double of any point of the invariant: X < 5.2, Y < 5.3, ZZ < 1.03, ZZZ < 1.02; pti_madd: X < 9.5, Y < 1.2,
//   ZZ < 1.03, ZZZ < 1.03 -- both inside the invariant, so the ladder and the digit walk are closed under it
//   a = ZZ ZZZ < 1 + rho' 5.6 = 1.04;  pre < 1 + rho' 1.04^2 = 1.01;  inv_fq(pre) < 1.01;  t, inv < 1.01
//   X ZZZ < 1 + rho' 20 = 1.12,  Y ZZ < 1 + rho' 16.8 = 1.10;  x, y < 1.01: multiplication outputs below 2 p, what
//   affi_pack and to_ext canonicalise
// G2, the invariant of bn254_ec2_29.hip.h (X < 1.21, Y < 13.4, ZZ < 3.2, ZZZ < 2.04 as maxima over the components; the
// tool carries c0 and c1 apart; Fq2::mul(a, b): c0 < 1 + rho' (A0 B0 + 32 A1), c1 < 1 + rho' (A0 B1 + A1 B0)):
//   a = ZZ ZZZ < 1.29;  pre = pre a < 1.21 at every step;  Fq2::inv(pre) < 1.21;  t = inv pre < 1.24,  inv = inv a < 1.24
//   X ZZZ < 1.25;  ZZ Y < 1.51 (Y is the SECOND operand: the 32 p lift of Fq2::mul multiplies the first one's c1, and
//   Y ZZ would reach 3.8);  x < 1.21,  y < 1.27: multiplication outputs below 2 p, what aff2_pack and to_ext canonicalise
//   These figures are for the points the additions produce (the tool's fixed point, c0 and c1 apart).  A record with
//   all eight components at the stated maxima at once is coarser: a < 1.65,  ZZ Y < 1.86,  y < 1.30, the rest as above
//   -- still multiplication outputs below 2 p (tools/g2_bounds.py: MUL_NORM_AT_INV; tests/test_mul_stages_host.py)
#pragma once
#include "compress_points.hip.h"
#include "device_common.hip.h"

namespace msm_amd {

enum : int { kMulBaseEach = 0, kMulBaseOne = 1 };
constexpr uint32_t kMulWindow = 8;                              // c of the fixed-base table
constexpr uint32_t kMulWindows = 254 / kMulWindow + 1;          // 32: one byte of the scalar per window
constexpr uint32_t kMulHalf = 1u << (kMulWindow - 1);           // entries per window
constexpr uint32_t kMulTableEntries = kMulWindows * kMulHalf;   // 4096
constexpr uint32_t kMulNormGroup = 16;                          // K: outputs that share one inversion
static_assert(kMulWindow == 8 && kMulWindows == 32, "mul_fixed reads one byte of the scalar per window");

// N 16-byte pieces between memory and registers (records of the library's own buffers: 16-byte aligned)
template <int QUADS>
MSM_HD void mul_load_quads(const void* p, uint32_t* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  MSM_UNROLL for (int i = 0; i < QUADS; ++i) {
    const uint4 v = q[i];
    dst[4 * i + 0] = v.x; dst[4 * i + 1] = v.y; dst[4 * i + 2] = v.z; dst[4 * i + 3] = v.w;
  }
#else
  memcpy(dst, p, 16 * QUADS);
#endif
}
template <int QUADS>
MSM_HD void mul_store_quads(void* p, const uint32_t* src) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = reinterpret_cast<uint4*>(p);
  MSM_UNROLL for (int i = 0; i < QUADS; ++i) q[i] = make_uint4(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]);
#else
  memcpy(p, src, 16 * QUADS);
#endif
}

// The canonical scalar s < r of one 32-byte record (layout: MSM_AMD_SCALAR_MONT_LE 0, _CANON_LE 1, _CANON_BE32 2), the
// rule of scalar_digits (k_sort.hip) and read_scalar (host_g2.hip).
MSM_HD u256 mul_scalar(int layout, const uint8_t* rec) {
  u256 k = check_u256(rec, 0, layout == 2);
  if (layout == 0) return Fr::from_mont(k);
  MSM_NO_UNROLL for (int i = 0; i < 5; ++i) k = Fr::reduce_once(k);   // 2^256 / r < 6
  return k;
}

// ---- G1 ------------------------------------------------------------------------------------------------------------
MSM_HD PtI pti_double_any(const PtI& p) { return pti_is_identity(p) ? p : pti_double(p); }
// acc + q, acc any XYZZ point, q affine and finite (q.y may be a negation < 4 p)
MSM_HD PtI pti_madd_any(const PtI& acc, const AffI& q) {
  if (pti_is_identity(acc)) return pti_from_affi(q);
  bool vanished = false;
  return pti_madd(acc, q, vanished);
}

struct MulG1 {
  using Aff = AffI;
  using Pt = PtI;
  using Packed = AffPacked;
  using F = fe29;
  static constexpr bool kG2 = false;

  MSM_HD static Aff aff_identity() { return AffI{Fq29::zero(), Fq29::zero()}; }
  MSM_HD static bool aff_is_identity(const Aff& a) { return affi_is_identity(a); }
  // One base record in the caller's layout -> canonical internal affine form; every identity encoding -> zero limbs.
  // The Jacobian layouts pay one inversion (x = X / Z^2, y = Y / Z^3).  Coordinates are taken as they are (no range or
  // curve check): any 256-bit value is a valid operand of from_ext.
  MSM_HD static Aff load_base(int layout, const uint8_t* rec) {
    Aff a = aff_identity();
    if (layout == kLayoutPrepared) {
      AffPacked q;
      q.x = check_u256(rec, 0);
      q.y = check_u256(rec, 8);
      return affi_unpack(q);
    }
    if (layout == kLayoutArkAffine && (check_word(rec, 16) & 0xFFu)) return a;
    const bool jac = layout == kLayoutArkProjective || layout == kLayoutJacBe32;
    const bool be = layout == kLayoutJacBe32;
    const u256 x = check_u256(rec, 0, be), y = check_u256(rec, 8, be);
    if (jac) {
      const u256 z = check_u256(rec, 16, be);
      if (u256_is_zero(z)) return a;
      const fe29 zi = Fq2::inv_fq(Fq29::from_ext(z));
      const fe29 zi2 = Fq29::sqr(zi);
      a.x = Fq29::mul(Fq29::from_ext(x), zi2);
      a.y = Fq29::mul(Fq29::from_ext(y), Fq29::mul(zi2, zi));
    } else {
      if (u256_is_zero(x) && u256_is_zero(y)) return a;
      a.x = Fq29::from_ext(x);
      a.y = Fq29::from_ext(y);
    }
    a.x = Fq29::canonical(a.x, 1);
    a.y = Fq29::canonical(a.y, 1);
    return a;
  }
  MSM_HD static Pt identity() { return pti_identity(); }
  MSM_HD static bool is_identity(const Pt& p) { return pti_is_identity(p); }
  MSM_HD static Pt double_any(const Pt& p) { return pti_double_any(p); }
  MSM_HD static Pt madd_any(const Pt& p, const Aff& q) { return pti_madd_any(p, q); }
  MSM_HD static Aff negate(const Aff& q) { return AffI{q.x, Fq29::neg(q.y)}; }
  // table entry of a point: to affine through the external Jacobian form (the path of build_tables_kernel)
  MSM_HD static Packed table_entry(const Pt& p) { return affi_pack(affi_from_ext(jac_to_affine(pti_to_ext(p)))); }
  MSM_HD static Packed load_packed(const Packed* t) {
    uint32_t w[16];
    mul_load_quads<4>(t, w);
    Packed r;
    MSM_UNROLL for (int i = 0; i < 8; ++i) {
      r.x.v[i] = w[i];
      r.y.v[i] = w[8 + i];
    }
    return r;
  }
  MSM_HD static void store_packed(Packed* t, const Packed& r) {
    uint32_t w[16];
    MSM_UNROLL for (int i = 0; i < 8; ++i) {
      w[i] = r.x.v[i];
      w[8 + i] = r.y.v[i];
    }
    mul_store_quads<4>(t, w);
  }
  MSM_HD static bool packed_is_identity(const Packed& r) { return affpacked_is_identity(r); }
  MSM_HD static Aff unpack_finite(const Packed& r) { return affi_unpack_finite(r); }
  MSM_HD static Pt load_pt(const Pt* p) {
    uint32_t w[36];
    mul_load_quads<9>(p, w);
    Pt r;
    MSM_UNROLL for (int i = 0; i < 9; ++i) {
      r.x.l[i] = w[i];
      r.y.l[i] = w[9 + i];
      r.zz.l[i] = w[18 + i];
      r.zzz.l[i] = w[27 + i];
    }
    return r;
  }
  MSM_HD static void store_pt(Pt* p, const Pt& a) {
    uint32_t w[36];
    MSM_UNROLL for (int i = 0; i < 9; ++i) {
      w[i] = a.x.l[i];
      w[9 + i] = a.y.l[i];
      w[18 + i] = a.zz.l[i];
      w[27 + i] = a.zzz.l[i];
    }
    mul_store_quads<9>(p, w);
  }
  // the field of the coordinates, for the shared inversion
  MSM_HD static F f_one() { return Fq29::one(); }
  MSM_HD static F f_zero() { return Fq29::zero(); }
  MSM_HD static F f_mul(const F& a, const F& b) { return Fq29::mul(a, b); }
  MSM_HD static F f_inv(const F& a) { return Fq2::inv_fq(a); }
  MSM_HD static void store_out(int layout, uint8_t* out, const Aff& a) { decompress_store_g1(layout, out, a); }
};

// ---- G2 ------------------------------------------------------------------------------------------------------------
struct MulG2 {
  using Aff = Aff2I;
  using Pt = PtI2;
  using Packed = Aff2Packed;
  using F = fq2;
  static constexpr bool kG2 = true;

  MSM_HD static Aff aff_identity() { return Aff2I{Fq2::zero(), Fq2::zero()}; }
  MSM_HD static bool aff_is_identity(const Aff& a) { return aff2i_is_identity(a); }
  MSM_HD static Aff load_base(int layout, const uint8_t* rec) {
    Aff a = aff_identity();
    const u256 x0 = check_u256(rec, 0), x1 = check_u256(rec, 8), y0 = check_u256(rec, 16), y1 = check_u256(rec, 24);
    if (layout == kG2LayoutPrepared) {
      const Aff2Packed q{x0, x1, y0, y1};
      return aff2packed_is_identity(q) ? a : aff2_unpack_finite(q);
    }
    if (layout == kG2LayoutArkAffine ? (check_word(rec, 32) & 0xFFu) != 0
                                     : (u256_is_zero(x0) && u256_is_zero(x1) && u256_is_zero(y0) && u256_is_zero(y1)))
      return a;
    a.x = fq2{Fq29::canonical(Fq29::from_ext(x0), 1), Fq29::canonical(Fq29::from_ext(x1), 1)};
    a.y = fq2{Fq29::canonical(Fq29::from_ext(y0), 1), Fq29::canonical(Fq29::from_ext(y1), 1)};
    return a;
  }
  MSM_HD static Pt identity() { return pt2_identity(); }
  MSM_HD static bool is_identity(const Pt& p) { return pt2_is_identity(p); }
  MSM_HD static Pt double_any(const Pt& p) { return pt2_double_any(p); }
  MSM_HD static Pt madd_any(const Pt& p, const Aff& q) { return pt2_madd_any(p, q); }
  MSM_HD static Aff negate(const Aff& q) { return Aff2I{q.x, Fq2::sub<4>(Fq2::zero(), q.y)}; }
  MSM_HD static Packed table_entry(const Pt& p) {
    return aff2_pack(pt2_is_identity(p) ? aff_identity() : pt2_to_affine(p));
  }
  MSM_HD static Packed load_packed(const Packed* t) {
    uint32_t w[32];
    mul_load_quads<8>(t, w);
    Packed r;
    MSM_UNROLL for (int i = 0; i < 8; ++i) {
      r.x0.v[i] = w[i];
      r.x1.v[i] = w[8 + i];
      r.y0.v[i] = w[16 + i];
      r.y1.v[i] = w[24 + i];
    }
    return r;
  }
  MSM_HD static void store_packed(Packed* t, const Packed& r) {
    uint32_t w[32];
    MSM_UNROLL for (int i = 0; i < 8; ++i) {
      w[i] = r.x0.v[i];
      w[8 + i] = r.x1.v[i];
      w[16 + i] = r.y0.v[i];
      w[24 + i] = r.y1.v[i];
    }
    mul_store_quads<8>(t, w);
  }
  MSM_HD static bool packed_is_identity(const Packed& r) { return aff2packed_is_identity(r); }
  MSM_HD static Aff unpack_finite(const Packed& r) { return aff2_unpack_finite(r); }
  MSM_HD static Pt load_pt(const Pt* p) {
    uint32_t w[72];
    mul_load_quads<18>(p, w);
    Pt r;
    MSM_UNROLL for (int i = 0; i < 9; ++i) {
      r.x.c0.l[i] = w[i];
      r.x.c1.l[i] = w[9 + i];
      r.y.c0.l[i] = w[18 + i];
      r.y.c1.l[i] = w[27 + i];
      r.zz.c0.l[i] = w[36 + i];
      r.zz.c1.l[i] = w[45 + i];
      r.zzz.c0.l[i] = w[54 + i];
      r.zzz.c1.l[i] = w[63 + i];
    }
    return r;
  }
  MSM_HD static void store_pt(Pt* p, const Pt& a) {
    uint32_t w[72];
    MSM_UNROLL for (int i = 0; i < 9; ++i) {
      w[i] = a.x.c0.l[i];
      w[9 + i] = a.x.c1.l[i];
      w[18 + i] = a.y.c0.l[i];
      w[27 + i] = a.y.c1.l[i];
      w[36 + i] = a.zz.c0.l[i];
      w[45 + i] = a.zz.c1.l[i];
      w[54 + i] = a.zzz.c0.l[i];
      w[63 + i] = a.zzz.c1.l[i];
    }
    mul_store_quads<18>(p, w);
  }
  MSM_HD static F f_one() { return Fq2::one(); }
  MSM_HD static F f_zero() { return Fq2::zero(); }
  MSM_HD static F f_mul(const F& a, const F& b) { return Fq2::mul(a, b); }
  MSM_HD static F f_inv(const F& a) { return Fq2::inv(a); }
  MSM_HD static void store_out(int layout, uint8_t* out, const Aff& a) { decompress_store_g2(layout, out, a); }
};

// ---- the bodies ------------------------------------------------------------------------------------------------------
// [k] a for the 256-bit integer k, a affine (identity: zero limbs).  Word j of k is picked by selects on the loop
// counter, bit b by a shift: no dynamically indexed array.
template <class G>
MSM_HD typename G::Pt mul_ladder(const typename G::Aff& a, const u256& k) {
  typename G::Pt acc = G::identity();
  if (G::aff_is_identity(a)) return acc;
  MSM_NO_UNROLL for (int j = 7; j >= 0; --j) {
    uint32_t e = 0;
    MSM_UNROLL for (int i = 0; i < 8; ++i) e = (i == j) ? k.v[i] : e;
    MSM_NO_UNROLL for (int b = 31; b >= 0; --b) {
      acc = G::double_any(acc);
      if ((e >> b) & 1u) acc = G::madd_any(acc, a);
    }
  }
  return acc;
}

// Entry e = w * kMulHalf + (d - 1) of the fixed-base table of a: [d 2^(c w)] a, packed.  d 2^(8 w) sits in one word of
// the 256-bit integer (d <= 128: d << 24 < 2^32).
template <class G>
MSM_HD typename G::Packed mul_table_entry(const typename G::Aff& a, uint32_t e) {
  const uint32_t w = e / kMulHalf, d = e % kMulHalf + 1u;
  u256 k;
  MSM_UNROLL for (uint32_t i = 0; i < 8; ++i) k.v[i] = (i == (w >> 2)) ? d << (8u * (w & 3u)) : 0u;
  return G::table_entry(mul_ladder<G>(a, k));
}

// [k] P from the table of P: the signed digits of k < r, least significant window first.
template <class G>
MSM_HD typename G::Pt mul_fixed(const u256& k, const typename G::Packed* table) {
  typename G::Pt acc = G::identity();
  uint32_t carry = 0;
  MSM_NO_UNROLL for (uint32_t j = 0; j < 8; ++j) {
    uint32_t e = 0;
    MSM_UNROLL for (uint32_t i = 0; i < 8; ++i) e = (i == j) ? k.v[i] : e;
    MSM_NO_UNROLL for (uint32_t b = 0; b < 4; ++b) {
      uint32_t v = ((e >> (8u * b)) & 0xFFu) + carry;
      const bool neg = v > kMulHalf;
      carry = neg ? 1u : 0u;
      if (neg) v = (1u << kMulWindow) - v;
      if (v == 0) continue;
      const typename G::Packed rec = G::load_packed(table + ((4u * j + b) * kMulHalf + (v - 1u)));
      if (G::packed_is_identity(rec)) continue;
      const typename G::Aff q = G::unpack_finite(rec);
      acc = G::madd_any(acc, neg ? G::negate(q) : q);
    }
  }
  return acc;
}

// XYZZ records [0, m) of `recs` (m <= kMulNormGroup) -> affine records in the output layout, one inversion (header).
// The records are overwritten.
template <class G>
MSM_HD void mul_normalise(typename G::Pt* recs, uint32_t m, int layout, uint32_t stride, uint8_t* out) {
  using F = typename G::F;
  F pre = G::f_one();
  MSM_NO_UNROLL for (uint32_t i = 0; i < m; ++i) {
    typename G::Pt p = G::load_pt(recs + i);
    const bool ident = G::is_identity(p);
    F a = G::f_one();
    if (ident) {
      p.x = G::f_zero();
      p.y = G::f_zero();
    } else {
      a = G::f_mul(p.zz, p.zzz);
      p.x = G::f_mul(p.x, p.zzz);
      p.y = G::f_mul(p.zz, p.y);
    }
    p.zz = a;
    p.zzz = pre;
    G::store_pt(recs + i, p);
    pre = G::f_mul(pre, a);
  }
  F inv = G::f_inv(pre);
  MSM_NO_UNROLL for (uint32_t i = m; i-- > 0;) {
    const typename G::Pt p = G::load_pt(recs + i);
    const F t = G::f_mul(inv, p.zzz);
    inv = G::f_mul(inv, p.zz);
    typename G::Aff r;
    r.x = G::f_mul(p.x, t);
    r.y = G::f_mul(p.y, t);
    G::store_out(layout, out + (size_t)i * stride, r);
  }
}

}  // namespace msm_amd
