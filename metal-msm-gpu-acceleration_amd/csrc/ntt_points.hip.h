// Transform over G1 points (msm_amd_ntt_points*, msm_amd_host_ntt_points): the bodies k_nttp.hip runs one lane per
// butterfly and host_nttp.hip runs on the CPU.  Everything here compiles for the device and for the host (MSM_HD).
//
// n = 2^L points, w the domain's root.  The network is decimation in time on a bit-reversed load:
//   load:   work[bitrev_L(j)] = in[j]                                    (nttp_load: MulG1::load_base, packed affine)
//   level l = 1 .. L, half = 2^(l-1), for every block base b (a multiple of 2^l) and every i < half:
//       u = work[b + i],  v = [w^(+-i n / 2^l)] work[b + i + half]       (- for INVERSE)
//       work[b + i] = u + v,  work[b + i + half] = u - v                 (nttp_bfly)
//   INVERSE: every record times n^-1 (nttp_scale)
// After L levels position k holds sum_i [w^(+-i k)] in[i], natural order.  Between two levels the records are packed
// affine (AffPacked, the bytes of MSM_AMD_POINT_PREPARED) in one of two work arrays: a level reads one array and writes
// XYZZ records that mul_normalise turns into the packed records of the other, so every addition is a mixed one.
//
// Twiddles.  The domain table holds w^j, j < n/2, Montgomery.  The exponent of lane i at level l is e = i << (L - l);
// FORWARD takes tw[e], INVERSE w^-e = -w^(n/2 - e) = r - tw[n/2 - e] for e != 0.  The ladder wants the integer, so the
// record leaves the Montgomery domain (Fr::from_mont).  e = 0 (all of level 1, i = 0 of every level) is the factor 1:
// no ladder, v is the record itself.
//
// Lanes (nttp_level, nttp_lane).  A level has n/2 butterflies = blocks * half, blocks = n / 2^l.  With at least
// kNttpUniformBlocks = 16 blocks the lanes run i-major (lane = i * blocks + block): 16 consecutive lanes share i, a whole
// wave does once there are 64 blocks -- the ladder's `if (bit)` is then wave-uniform and the i = 0 waves run no ladder.
// Below 16 blocks the lanes run block-major (lane = block * half + i).  Either way a run of `group` = 16 consecutive
// lanes (fewer when the level is narrower: min(16, half) in block-major order) writes its upper outputs, and its lower
// ones, to positions in arithmetic progression: stride 2^l records i-major, 1 block-major.  That is what lets
// mul_normalise, which writes consecutive records at one stride, take them: a chunk of m lanes from lane0 (m and lane0
// multiples of `group`) keeps the m upper outputs in XYZZ records [0, m) and the m lower ones in [m, 2 m), and the
// normalisation group g covers records [g group, (g + 1) group) (nttp_group).  The groups only decide which records
// share an inversion; the output is canonical, so no byte depends on the chunk or on the order.
//
// Cost.  A laddered butterfly is 256 doublings and about 127 mixed additions, roughly 4 000 field products, against two
// 64-byte reads and two 144-byte writes: the levels are bound by VALU issue, not by memory, and nothing is staged in LDS.
//
// Bounds (multiples of p; tools/fq29_bounds.py: ntt_points re-derives them).  Everything stays inside the invariant of
// bn254_ec29.hip.h (X < 10, Y < 6, ZZ < 2.8, ZZZ < 2, limbs 0..7 < 2^29 + 8):
//   u, q: unpacked records, canonical, exact 29-bit limbs
//   T = mul_ladder(q, k) or pti_from_affi(q): a point of the invariant (mul_points.hip.h), Y up to 5.3 after a doubling
//   the negated T.  Fq29::neg takes values below 3.9 p, a Y of the invariant reaches 6 p.  So Y is first multiplied by
//     one: Y' = Y one / rho < 1 + rho' 6 = 1.04, then -Y' = 4 p - Y' < 4 p, normalised (Fq29::neg) -- inside Y < 6.  One
//     product per butterfly next to 4 000; X, ZZ, ZZZ are T's own.
//   u + T, u - T = pti_madd_any(T or -T, u): the accumulator is a point of the invariant, the affine operand canonical
//     -- the case of pti_madd in the ladder itself, with its doubling (T = u) and vanishing (T = -u) branches; outputs
//     X < 9.5, Y < 1.2 (doubling: 5.3), ZZ, ZZZ < 1.03
//   an identity u hands T and -T through; an identity q makes T the identity and both outputs pti_from_affi(u)
//   nttp_scale: mul_ladder on a canonical base, as mul_each_kernel
#pragma once
#include "mul_points.hip.h"
#include "ntt.hip.h"

namespace msm_amd {

constexpr uint32_t kNttpUniformBlocks = 16;   // a level with at least this many blocks runs its lanes i-major
constexpr uint32_t kNttpAllLevels = ~0u;
static_assert(kNttpUniformBlocks == kMulNormGroup, "a normalisation group of i-major lanes shares its i");

struct NttpLevel {
  uint32_t log_n, level;   // l = 1 .. log_n
  uint32_t log_half;       // l - 1
  uint32_t log_blocks;     // log_n - l
  uint32_t imajor;         // lane = i * blocks + block; else lane = block * half + i
  uint32_t group;          // lanes per normalisation group: a power of two <= kMulNormGroup
};

MSM_HD NttpLevel nttp_level(uint32_t log_n, uint32_t level) {
  NttpLevel v;
  v.log_n = log_n, v.level = level;
  v.log_half = level - 1u, v.log_blocks = log_n - level;
  v.imajor = (1u << v.log_blocks) >= kNttpUniformBlocks ? 1u : 0u;
  const uint32_t half = 1u << v.log_half;
  v.group = v.imajor ? kMulNormGroup : (half < kMulNormGroup ? half : kMulNormGroup);
  return v;
}

// lane < n/2 of a level -> i and the position of the upper record b + i (the lower one is at + half)
MSM_HD uint32_t nttp_lane(const NttpLevel& v, uint32_t lane, uint32_t& i) {
  uint32_t block;
  if (v.imajor) {
    i = lane >> v.log_blocks;
    block = lane & ((1u << v.log_blocks) - 1u);
  } else {
    block = lane >> v.log_half;
    i = lane & ((1u << v.log_half) - 1u);
  }
  return (block << v.level) + i;
}

// Normalisation group g of a chunk of m lanes from lane0: its `group` XYZZ records start at record g * group of the
// chunk; the first one goes to position `pos` of the level's output, the next ones follow at `stride` records.
MSM_HD void nttp_group(const NttpLevel& v, uint32_t lane0, uint32_t m, uint32_t g, uint32_t& pos, uint32_t& stride) {
  const uint32_t q0 = g * v.group;
  const bool lower = q0 >= m;
  uint32_t i;
  pos = nttp_lane(v, lane0 + (lower ? q0 - m : q0), i) + (lower ? 1u << v.log_half : 0u);
  stride = v.imajor ? 1u << v.level : 1u;
}

// The factor of lane i at level l as the INTEGER the ladder walks; false: the factor is 1 (tw is not read).
MSM_HD bool nttp_twiddle(const u256* tw, const NttpLevel& v, int direction, uint32_t i, u256& k) {
  if (i == 0) return false;
  const uint32_t e = i << v.log_blocks;   // < n/2
  k = direction == kNttInverse ? Fr::neg(tw[(1u << (v.log_n - 1u)) - e]) : tw[e];
  k = Fr::from_mont(k);
  return true;
}

// -T of an XYZZ point of the invariant (header: Y through one product, then Fq29::neg)
MSM_HD PtI nttp_negate(const PtI& t) {
  if (pti_is_identity(t)) return t;
  PtI r = t;
  r.y = Fq29::neg(Fq29::mul(t.y, Fq29::one()));
  return r;
}

// T = [k] q (laddered) or q itself, q a packed record
template <class G>
MSM_HD typename G::Pt nttp_factor(const typename G::Packed& qr, bool laddered, const u256& k) {
  if (G::packed_is_identity(qr)) return G::identity();
  const typename G::Aff q = G::unpack_finite(qr);
  return laddered ? mul_ladder<G>(q, k) : G::madd_any(G::identity(), q);
}

// xyzz_s <- u + T, xyzz_d <- u - T, u a packed record.  The sum is stored before the difference is formed: one result
// lives in registers at a time.
MSM_HD void nttp_bfly(const AffPacked& ur, const PtI& t, PtI* xyzz_s, PtI* xyzz_d) {
  if (affpacked_is_identity(ur)) {
    MulG1::store_pt(xyzz_s, t);
    MulG1::store_pt(xyzz_d, nttp_negate(t));
    return;
  }
  const AffI u = affi_unpack_finite(ur);
  MulG1::store_pt(xyzz_d, t);                    // T waits in the record of the difference while the sum is formed
  MulG1::store_pt(xyzz_s, pti_madd_any(t, u));
  MulG1::store_pt(xyzz_d, pti_madd_any(nttp_negate(MulG1::load_pt(xyzz_d)), u));
}

// One butterfly of a level: reads src (packed), writes the two XYZZ records.
MSM_HD void nttp_butterfly(const AffPacked* src, const u256* tw, const NttpLevel& v, int direction, uint32_t lane,
                           PtI* xyzz_s, PtI* xyzz_d) {
  uint32_t i;
  const uint32_t pos = nttp_lane(v, lane, i);
  u256 k = u256_zero();
  const bool laddered = nttp_twiddle(tw, v, direction, i, k);
  const PtI t = nttp_factor<MulG1>(MulG1::load_packed(src + pos + (1u << v.log_half)), laddered, k);
  nttp_bfly(MulG1::load_packed(src + pos), t, xyzz_s, xyzz_d);   // u is read behind the ladder: its registers are free until here
}

// The load pass: record j of the caller -> packed affine at the bit-reversed index
MSM_HD void nttp_load(int layout_in, uint32_t stride, const uint8_t* in, uint32_t log_n, uint32_t j, AffPacked* work) {
  MulG1::store_packed(work + ntt_bitrev(j, log_n), affi_pack(MulG1::load_base(layout_in, in + (size_t)j * stride)));
}

// The uniform-scalar pass: [k] record, or the record itself as an XYZZ point (laddered false: k = 1)
MSM_HD PtI nttp_scale(const AffPacked* src, uint32_t pos, bool laddered, const u256& k) {
  return nttp_factor<MulG1>(MulG1::load_packed(src + pos), laddered, k);
}

// n^-1 mod r as an integer (host only); false for n = 1: the factor is 1
inline bool nttp_n_inv(uint32_t log_n, u256* k) {
  if (log_n == 0) return false;
  u256 n = u256_zero();
  n.v[log_n >> 5] = 1u << (log_n & 31);
  *k = Fr::from_mont(ntt_fr_inv(Fr::to_mont(n)));
  return true;
}

}  // namespace msm_amd
