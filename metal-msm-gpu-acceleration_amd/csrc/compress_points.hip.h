// Compressed points (msm_amd_decompress_points*, msm_amd_compress_points*, their G2 forms and host twins): the
// per-record bodies that k_compress.hip runs one lane per record and host_compress.hip runs on the CPU.
//
// Wire formats (include/msm_amd.h states the rules in full).  x is the CANONICAL integer, little-endian, 32 B (G2:
// x.c0 then x.c1, 64 B); the top two bits of the last byte carry the flags:
//   kCompressedArk     0x80 = y is the larger of {y, p - y}, 0x40 = identity;  Fq2 order: c1 first, c0 on a tie
//   kCompressedParity  0x80 = identity, 0x40 = sign(y): lsb of y (G2: of y.c0, or of y.c1 when y.c0 = 0)
// A record gets ONE reason code, the first rule that fails: 4 BAD_ENCODING (both flags, or the identity flag with a
// non-zero bit of x), 1 NOT_REDUCED (x, or a component of it, >= p), 2 NOT_ON_CURVE (x^3 + b has no square root).
//
// Fq square root.  p = 3 mod 4: r = a^((p + 1) / 4), accepted iff r^2 == a (is_zero_exact of the difference).  The
// exponent is a constant of 252 bits, walked most significant first in 2-bit windows over the table {a, a^2, a^3}:
// 256 squarings, 88 window products, 2 table products (the binary ladder needs 109 products; a 4-bit window needs 71
// but its 15-entry table is 135 registers per lane, or a dynamically indexed array, i.e. scratch).  The window is a
// compile-time constant per trip, the same for all lanes: the table entry is picked by selects on a uniform value and
// the loops are not unrolled.
// Bounds (multiples of p, rho' = p / rho = 0.0059; tools/g2_bounds.py re-derives them):
//   operand a: normalised, value < 8 p.   a^2 < 1 + rho' 64 = 1.38,  a^3 < 1 + rho' 1.38 * 8 = 1.07
//   running power r: < 1.01 after the two squarings, < 1 + rho' 1.01 * 8 = 1.05 after a window product: every operand
//   is a valid one; the result is < 1.05 p
//   acceptance: r^2 - a + 8 p < 9.02 p, normalised, decided by is_zero_exact
// Fq2 square root of a = a0 + a1 u (components normalised, < 4 p), two ladders and one inversion for every lane:
//   z = (a1 == 0);   r1 = sqrt(z ? a0 : a0^2 + a1^2)       (norm < 1 + rho' 2 * 16 = 1.19)
//   r2 = sqrt(z ? -a0 : (a0 + r1) / 2)                     (-a0 = 4 p - a0 <= 4 p;  (a0 + r1) / 2 = (a0 + r1) * (rho / 2)
//                                                           / rho < 1 + rho' 5.05 = 1.03)
//   z:  root = (r1, 0) if r1^2 == a0, else (0, r2)         (-1 is a non-residue: -a0 is a square when a0 is not)
//   !z: w = a1 / (2 r2) (2 r2 < 2.1 p, inv_fq < 1.2 p, w < 1 + rho' 4 * 1.2 = 1.03);
//       root = (r2, w) if r2^2 == (a0 + r1) / 2, else (w, r2)     (then r2^2 == -(a0 + r1) / 2)
//   accepted iff root^2 == a (Fq2::sqr, sub<8>, is_zero_exact): a norm without a root, or a wrong candidate, fails here.
// Sign selection works on the canonical INTEGER y = canonical(mul(y, 1)) (mul by the integer 1 leaves the Montgomery
// domain: < p (1 + 2^-250)); the other root is squash(neg(y)) < 1 + rho' 4 = 1.03 p.  Every coordinate handed to a
// packer (affi_pack, aff2_pack, to_ext) is a multiplication output below 2 p or exact zero limbs.
#pragma once
#include "bn254_ec29.hip.h"
#include "check_points.hip.h"

namespace msm_amd {

enum : int { kCompressedArk = 0, kCompressedParity = 1 };

MSM_HD constexpr uint32_t comp_const(int which, int i) {
  constexpr uint32_t c[2][9] = {
      // rho^2 mod p: canonical integer -> internal domain
      {0x059BAC10u, 0x0D1503A3u, 0x018016B8u, 0x10AB0CA8u, 0x02632639u, 0x02C0169Fu, 0x169BFD53u, 0x11869D4Cu, 0x002A11A6u},
      // rho / 2 mod p: halving inside the domain
      {0x16FCE4B4u, 0x0A904407u, 0x0A626A11u, 0x12109375u, 0x1014A498u, 0x100EC0C7u, 0x093E16A4u, 0x09C376EEu, 0x001F1642u}};
  return c[which][i];
}
MSM_HD fe29 comp_fe(int which) {
  fe29 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) r.l[i] = comp_const(which, i);
  return r;
}
// (p + 1) / 4 and (p - 1) / 2 as 8 x u32, little-endian
MSM_HD constexpr uint32_t comp_sqrt_exp(int i) {
  constexpr uint32_t c[8] = {0xB61F3F52u, 0x4F082305u, 0x5A1C72A3u, 0x65E05AA4u, 0xA0605617u, 0x6E14116Du, 0xB84C680Au, 0x0C19139Cu};
  return c[i];
}
MSM_HD constexpr uint32_t comp_half_p(int i) {
  constexpr uint32_t c[8] = {0x6C3E7EA3u, 0x9E10460Bu, 0xB438E546u, 0xCBC0B548u, 0x40C0AC2Eu, 0xDC2822DBu, 0x7098D014u, 0x18322739u};
  return c[i];
}

// ---- roots ---------------------------------------------------------------------------------------------------------
// a^((p + 1) / 4); a normalised, < 8 p (header).  Result < 1.05 p.
MSM_HD fe29 comp_sqrt_candidate(const fe29& a) {
  const fe29 a2 = Fq29::sqr(a);
  const fe29 a3 = Fq29::mul(a2, a);
  fe29 r = Fq29::one();
  MSM_NO_UNROLL for (int j = 7; j >= 0; --j) {
    uint32_t e = 0;   // word j of the exponent, an immediate
    MSM_UNROLL for (int k = 0; k < 8; ++k) e = (k == j) ? comp_sqrt_exp(k) : e;
    MSM_NO_UNROLL for (int b = 30; b >= 0; b -= 2) {
      r = Fq29::sqr(Fq29::sqr(r));
      const uint32_t w = (e >> b) & 3u;
      if (w) {
        fe29 m;
        MSM_UNROLL for (int i = 0; i < 9; ++i) m.l[i] = (w == 1u) ? a.l[i] : (w == 2u) ? a2.l[i] : a3.l[i];
        r = Fq29::mul(r, m);
      }
    }
  }
  return r;
}
MSM_HD bool comp_is_root(const fe29& r, const fe29& a) {
  return Fq29::is_zero_exact(Fq29::norm(Fq29::sub<K8E30>(Fq29::sqr(r), a)));
}
// root of a if there is one (then true); a normalised, < 8 p
MSM_HD bool comp_sqrt_fq(const fe29& a, fe29& root) {
  root = comp_sqrt_candidate(a);
  return comp_is_root(root, a);
}

MSM_HD fe29 comp_select(bool c, const fe29& a, const fe29& b) {
  fe29 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}

// root of a in Fq2 if there is one (then true); components normalised, < 4 p (header)
MSM_HD bool comp_sqrt_fq2(const fq2& a, fq2& root) {
  const bool z = Fq29::is_zero_exact(a.c1);
  const fe29 in1 = comp_select(z, a.c0, Fq2::norm_fq(a));
  fe29 r1;
  const bool ok1 = comp_sqrt_fq(in1, r1);
  const fe29 half = Fq29::mul(Fq29::norm(Fq29::add(a.c0, r1)), comp_fe(1));
  const fe29 in2 = comp_select(z, Fq2::sub1<4>(Fq29::zero(), a.c0), half);
  fe29 r2;
  const bool ok2 = comp_sqrt_fq(in2, r2);
  const fe29 w = Fq29::mul(a.c1, Fq2::inv_fq(Fq29::norm(Fq29::add(r2, r2))));
  const bool real_first = z ? ok1 : ok2;   // which component the ladder's root is
  root.c0 = real_first ? (z ? r1 : r2) : (z ? Fq29::zero() : w);
  root.c1 = real_first ? (z ? Fq29::zero() : w) : r2;
  return Fq2::is_zero_exact(Fq2::sub<8>(Fq2::sqr(root), a));
}

// ---- sign rules ----------------------------------------------------------------------------------------------------
// canonical integer of an internal value (a multiplication output), as limbs
MSM_HD fe29 comp_canonical_int(const fe29& a) {
  fe29 o = Fq29::zero();
  o.l[0] = 1u;
  return Fq29::canonical(Fq29::mul(a, o), 1);
}
MSM_HD bool comp_gt_half(const u256& y) {   // y > (p - 1) / 2, i.e. y > p - y
  u256 h, d;
  MSM_UNROLL for (int i = 0; i < 8; ++i) h.v[i] = comp_half_p(i);
  return u256_sub(d, h, y) != 0;
}
// the flag bit of y under the format's rule (canonical integers)
MSM_HD uint32_t comp_sign_fq(int format, const u256& y) {
  return format == kCompressedArk ? (comp_gt_half(y) ? 1u : 0u) : (y.v[0] & 1u);
}
MSM_HD uint32_t comp_sign_fq2(int format, const u256& y0, const u256& y1) {
  if (format == kCompressedArk) return (u256_is_zero(y1) ? comp_gt_half(y0) : comp_gt_half(y1)) ? 1u : 0u;
  return (u256_is_zero(y0) ? y1.v[0] : y0.v[0]) & 1u;
}
MSM_HD fe29 comp_neg(const fe29& y) { return Fq29::mul(Fq29::neg(y), Fq29::one()); }

// ---- stores ----------------------------------------------------------------------------------------------------------
// records of the ark layouts are only 8-byte aligned: 8-byte stores throughout
MSM_HD void comp_store_u256(uint8_t* dst, const u256& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint2* q = reinterpret_cast<uint2*>(dst);
  MSM_UNROLL for (int i = 0; i < 4; ++i) q[i] = make_uint2(a.v[2 * i], a.v[2 * i + 1]);
#else
  memcpy(dst, a.v, 32);
#endif
}
MSM_HD void comp_store_flag(uint8_t* dst, uint32_t flag) {   // the infinity byte of an ark affine record and its padding
  u256 t = u256_zero();
  t.v[0] = flag;
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint2*>(dst) = make_uint2(t.v[0], 0u);
#else
  memcpy(dst, t.v, 8);
#endif
}
MSM_HD u256 comp_all_ones() {
  u256 r;
  MSM_UNROLL for (int i = 0; i < 8; ++i) r.v[i] = 0xFFFFFFFFu;
  return r;
}

// ---- decompression ---------------------------------------------------------------------------------------------------
// flags of the word that holds the last byte: (identity flag, sign flag)
MSM_HD void comp_flags(int format, uint32_t top_word, bool& both, bool& ident, uint32_t& sign) {
  const uint32_t f = top_word >> 30;   // bit 1 = 0x80, bit 0 = 0x40
  both = f == 3u;
  ident = format == kCompressedArk ? (f & 1u) != 0 : (f >> 1) != 0;
  sign = format == kCompressedArk ? (f >> 1) : (f & 1u);
}

// One compressed G1 record -> reason code and the point in the internal affine form (exact zero limbs for the identity
// and for every invalid record).
MSM_HD uint32_t decompress_record_g1(int format, const uint8_t* rec, AffI& pt, bool& identity) {
  identity = false;
  pt.x = Fq29::zero();
  pt.y = Fq29::zero();
  u256 x = check_u256(rec, 0);
  bool both, ident;
  uint32_t sign;
  comp_flags(format, x.v[7], both, ident, sign);
  x.v[7] &= 0x3FFFFFFFu;
  if (both || (ident && !u256_is_zero(x))) return kPointBadEncoding;
  if (ident) {
    identity = true;
    return kPointValid;
  }
  if (check_ge_p(x)) return kPointNotReduced;
  const fe29 xi = Fq29::mul(Fq29::unpack256(x), comp_fe(0));
  const fe29 rhs = Fq29::norm(Fq29::add(Fq29::mul(Fq29::sqr(xi), xi), check_b_g1()));   // < 2.02 p
  fe29 y;
  if (!comp_sqrt_fq(rhs, y)) return kPointNotOnCurve;
  if (comp_sign_fq(format, Fq29::pack256(comp_canonical_int(y))) != sign) y = comp_neg(y);
  pt.x = xi;
  pt.y = y;
  return kPointValid;
}

// The point in the caller's output layout: MSM_AMD_POINT_H2C_AFFINE (64 B), _ARK_AFFINE (72 B), _PREPARED (64 B, the
// record convert_bases writes: affi_pack)
MSM_HD void decompress_store_g1(int layout, uint8_t* out, const AffI& pt) {
  if (layout == kLayoutPrepared) {
    const AffPacked r = affi_pack(pt);
    comp_store_u256(out, r.x);
    comp_store_u256(out + 32, r.y);
    return;
  }
  comp_store_u256(out, Fq29::to_ext(pt.x));   // zero limbs -> zero
  comp_store_u256(out + 32, Fq29::to_ext(pt.y));
  if (layout == kLayoutArkAffine) comp_store_flag(out + 64, affi_is_identity(pt) ? 1u : 0u);
}

MSM_HD uint32_t decompress_record_g2(int format, const uint8_t* rec, Aff2I& pt, bool& identity) {
  identity = false;
  pt.x = Fq2::zero();
  pt.y = Fq2::zero();
  const u256 x0 = check_u256(rec, 0);
  u256 x1 = check_u256(rec, 8);
  bool both, ident;
  uint32_t sign;
  comp_flags(format, x1.v[7], both, ident, sign);
  x1.v[7] &= 0x3FFFFFFFu;
  if (both || (ident && !(u256_is_zero(x0) && u256_is_zero(x1)))) return kPointBadEncoding;
  if (ident) {
    identity = true;
    return kPointValid;
  }
  if (check_ge_p(x0) || check_ge_p(x1)) return kPointNotReduced;
  const fq2 xi = fq2{Fq29::mul(Fq29::unpack256(x0), comp_fe(0)), Fq29::mul(Fq29::unpack256(x1), comp_fe(0))};
  const fq2 rhs = Fq2::norm(Fq2::add(Fq2::mul(Fq2::sqr(xi), xi), check_g2_fq2(0)));   // < 2.21 p per component
  fq2 y;
  if (!comp_sqrt_fq2(rhs, y)) return kPointNotOnCurve;
  const u256 y0 = Fq29::pack256(comp_canonical_int(y.c0)), y1 = Fq29::pack256(comp_canonical_int(y.c1));
  if (comp_sign_fq2(format, y0, y1) != sign) y = fq2{comp_neg(y.c0), comp_neg(y.c1)};
  pt.x = xi;
  pt.y = y;
  return kPointValid;
}

// MSM_AMD_G2_POINT_H2C_AFFINE (128 B), _ARK_AFFINE (136 B), _PREPARED (128 B, the record convert_bases_g2 writes)
MSM_HD void decompress_store_g2(int layout, uint8_t* out, const Aff2I& pt) {
  if (layout == kG2LayoutPrepared) {
    const Aff2Packed r = aff2_pack(pt);
    comp_store_u256(out, r.x0);
    comp_store_u256(out + 32, r.x1);
    comp_store_u256(out + 64, r.y0);
    comp_store_u256(out + 96, r.y1);
    return;
  }
  comp_store_u256(out, Fq29::to_ext(pt.x.c0));
  comp_store_u256(out + 32, Fq29::to_ext(pt.x.c1));
  comp_store_u256(out + 64, Fq29::to_ext(pt.y.c0));
  comp_store_u256(out + 96, Fq29::to_ext(pt.y.c1));
  if (layout == kG2LayoutArkAffine) comp_store_flag(out + 128, aff2i_is_identity(pt) ? 1u : 0u);
}

// ---- compression -----------------------------------------------------------------------------------------------------
// flag bits of the last word: identity record / sign bit of a finite point
MSM_HD uint32_t comp_flag_word(int format, bool ident, uint32_t sign) {
  if (ident) return format == kCompressedArk ? 0x40000000u : 0x80000000u;
  return sign ? (format == kCompressedArk ? 0x80000000u : 0x40000000u) : 0u;
}

// One affine G1 record (MSM_AMD_POINT_H2C_AFFINE / _ARK_AFFINE) -> 32 bytes; true if a stored coordinate was >= p (the
// record is then all 0xFF).  Points are not checked for being on the curve.
MSM_HD bool compress_record_g1(int layout, const uint8_t* rec, int format, uint8_t* out) {
  const u256 x = check_u256(rec, 0), y = check_u256(rec, 8);
  u256 r = u256_zero();
  if (layout == kLayoutArkAffine ? (check_word(rec, 16) & 0xFFu) != 0 : (u256_is_zero(x) && u256_is_zero(y))) {
    r.v[7] = comp_flag_word(format, true, 0);
    comp_store_u256(out, r);
    return false;
  }
  if (check_ge_p(x) || check_ge_p(y)) {
    comp_store_u256(out, comp_all_ones());
    return true;
  }
  r = Fq::from_mont(x);
  r.v[7] |= comp_flag_word(format, false, comp_sign_fq(format, Fq::from_mont(y)));
  comp_store_u256(out, r);
  return false;
}

// One affine G2 record (MSM_AMD_G2_POINT_H2C_AFFINE / _ARK_AFFINE) -> 64 bytes
MSM_HD bool compress_record_g2(int layout, const uint8_t* rec, int format, uint8_t* out) {
  const u256 x0 = check_u256(rec, 0), x1 = check_u256(rec, 8), y0 = check_u256(rec, 16), y1 = check_u256(rec, 24);
  u256 r = u256_zero();
  if (layout == kG2LayoutArkAffine ? (check_word(rec, 32) & 0xFFu) != 0
                                   : (u256_is_zero(x0) && u256_is_zero(x1) && u256_is_zero(y0) && u256_is_zero(y1))) {
    comp_store_u256(out, r);
    r.v[7] = comp_flag_word(format, true, 0);
    comp_store_u256(out + 32, r);
    return false;
  }
  if (check_ge_p(x0) || check_ge_p(x1) || check_ge_p(y0) || check_ge_p(y1)) {
    comp_store_u256(out, comp_all_ones());
    comp_store_u256(out + 32, comp_all_ones());
    return true;
  }
  comp_store_u256(out, Fq::from_mont(x0));
  r = Fq::from_mont(x1);
  r.v[7] |= comp_flag_word(format, false, comp_sign_fq2(format, Fq::from_mont(y0), Fq::from_mont(y1)));
  comp_store_u256(out + 32, r);
  return false;
}

// ---- raw-limb root ops (MSM_AMD_RAW_FE_SQRT, MSM_AMD_G2_RAW_FQ2_SQRT) --------------------------------------------------
// a: 36 words (a0 = words 0..8), out: 40 words: root in 0..8, word 9 = 1 if there is one
MSM_HD void raw_sqrt_fq(const uint32_t* a, uint32_t* out) {
  fe29 v, r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) v.l[i] = a[i];
  const bool ok = comp_sqrt_fq(v, r);
  MSM_UNROLL for (int i = 0; i < 40; ++i) out[i] = 0;
  MSM_UNROLL for (int i = 0; i < 9; ++i) out[i] = ok ? r.l[i] : 0u;
  out[9] = ok ? 1u : 0u;
}
// a: 72 words (fq2 = words 0..17), out: 80 words: root in 0..17, word 72 = 1 if there is one
MSM_HD void raw_sqrt_fq2(const uint32_t* a, uint32_t* out) {
  fq2 v, r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) {
    v.c0.l[i] = a[i];
    v.c1.l[i] = a[9 + i];
  }
  const bool ok = comp_sqrt_fq2(v, r);
  MSM_UNROLL for (int i = 0; i < 80; ++i) out[i] = 0;
  MSM_UNROLL for (int i = 0; i < 9; ++i) {
    out[i] = ok ? r.c0.l[i] : 0u;
    out[9 + i] = ok ? r.c1.l[i] : 0u;
  }
  out[72] = ok ? 1u : 0u;
}

}  // namespace msm_amd
