// Scalars of bounded width (msm_amd_msm_bounded*, msm_amd_scalar_width*): the magnitude of a residue, its bit length and
// the argument checks, shared by the digit kernels (k_sort.hip), the host driver (msm_host.hip) and the host twins
// (host_msm.hip, host_g2.hip).
//   value     : the residue s mod r of a record (MONT_LE de-Montgomeryed, raw CANON_LE words reduced first)
//   unsigned  : magnitude s
//   signed    : magnitude min(s, r - s); the record is negative when s > (r - 1) / 2, and then -magnitude = s mod r:
//               the MSM adds magnitude * (-P), which the signed digits carry as a flipped sign per digit
// A call with the bound `bits` takes magnitudes below 2^bits and plans bits / c + 1 digit windows: the top window
// holds bits - (W - 1) c <= c - 1 bits, so with the carry of the window below it stays <= 2^(c-1) and never carries out.
#pragma once
#include "bn254_fq.hip.h"
#include "../../include/msm_amd.h"

namespace msm_amd {

constexpr uint32_t kScalarBits = 254;          // bit length of r
constexpr uint32_t kScalarBitsSigned = 253;    // bit length of (r - 1) / 2: a signed bound of 253 takes every residue

// The width of a plan: bits == 0 is the unbounded call (full width, unsigned, nothing to check).
struct WidthBound {
  uint32_t bits = 0;
  uint32_t sign = 0;
  bool bounded() const { return bits != 0; }
  // every residue fits: no record can violate the bound (the check is skipped; unsigned 254 is the unbounded call)
  bool total() const { return bits == 0 || bits >= (sign ? kScalarBitsSigned : kScalarBits); }
  uint32_t width() const { return bits ? bits : kScalarBits; }
};

inline const char* width_sign_check(int sign) {
  return (sign == MSM_AMD_WIDTH_UNSIGNED || sign == MSM_AMD_WIDTH_SIGNED)
             ? nullptr
             : "sign must be MSM_AMD_WIDTH_UNSIGNED or MSM_AMD_WIDTH_SIGNED";
}
// driver and twins alike: null on valid (bits, sign)
inline const char* width_bound_check(uint32_t bits, int sign) {
  if (const char* why = width_sign_check(sign)) return why;
  if (bits < 1 || bits > (sign ? kScalarBitsSigned : kScalarBits))
    return "bits must be 1..254 (MSM_AMD_WIDTH_UNSIGNED) or 1..253 (MSM_AMD_WIDTH_SIGNED)";
  return nullptr;
}
inline const char* width_layout_check(int scalar_layout) {
  return (scalar_layout == MSM_AMD_SCALAR_MONT_LE || scalar_layout == MSM_AMD_SCALAR_CANON_LE)
             ? nullptr
             : "scalar layout must be MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE";
}

// msm_amd_scalar_width*, msm_amd_host_scalar_width: null on valid arguments (stats is optional)
inline const char* scalar_width_check(int scalar_layout, const void* scalars, size_t n, int sign, const uint32_t* bits) {
  if (const char* why = width_layout_check(scalar_layout)) return why;
  if (const char* why = width_sign_check(sign)) return why;
  if (!bits) return "bits is null";
  if (n > 0 && !scalars) return "null pointer with n > 0";
  if (n > 0xFFFFFFFFull) return "n >= 2^32";
  return nullptr;
}

// the residue of a record as the digit kernels read it
MSM_HD u256 scalar_residue(u256 k, int scalars_mont) {
  if (scalars_mont) return Fr::from_mont(k);
  // raw 256-bit words: 2^256 / r < 6, at most five subtractions
  for (int i = 0; i < 5; ++i) k = Fr::reduce_once(k);
  return k;
}

// signed fold of a residue k < r: *neg = 1 and r - k when r - k < k (r is odd: k > (r - 1) / 2), else k itself
MSM_HD u256 scalar_magnitude(const u256& k, uint32_t sign, uint32_t* neg) {
  u256 m, d;
  u256_sub(m, Fr::modulus(), k);
  const uint32_t flip = sign ? u256_sub(d, m, k) : 0u;   // borrow: r - k < k
  u256 r;
  MSM_UNROLL for (int i = 0; i < 8; ++i) r.v[i] = flip ? m.v[i] : k.v[i];
  *neg = flip;
  return r;
}

// bit length (0 for zero): the highest non-zero word and a count-leading-zeros of it
MSM_HD uint32_t u256_bit_length(const u256& a) {
  uint32_t len = 0;
  MSM_UNROLL for (int i = 0; i < 8; ++i) {
    const uint32_t w = a.v[i];
    if (w) len = 32u * (uint32_t)i + 32u - (uint32_t)__builtin_clz(w);
  }
  return len;
}

// what a width scan reports; merge folds the scan of the records BEHIND a's into a (a tie keeps the lower index)
struct WidthStats {
  uint32_t bits = 0;
  uint64_t zeros = 0, negatives = 0, widest = 0;
};
inline void width_stats_merge(WidthStats& a, const WidthStats& b) {
  if (b.bits > a.bits) a.bits = b.bits, a.widest = b.widest;
  a.zeros += b.zeros;
  a.negatives += b.negatives;
}
// stats[4]: zero records, negative records, lowest index of a widest record, 0
inline void scalar_width_out(const WidthStats& r, uint32_t* bits, uint64_t* stats) {
  *bits = r.bits;
  if (stats) stats[0] = r.zeros, stats[1] = r.negatives, stats[2] = r.widest, stats[3] = 0;
}

}  // namespace msm_amd
