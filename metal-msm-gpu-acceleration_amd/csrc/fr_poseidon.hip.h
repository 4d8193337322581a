// Poseidon over BN254 Fr (msm_amd_poseidon_*): the permutation of Grassi et al. with the S-box x^5 for a state of t = 2 .. 5
// records, the hash and the Merkle trees built on it: the bodies shared by the kernels (k_fr.hip), the host twins
// (host_fr.hip) and the host driver (msm_host.hip).  Everything here compiles for the device and for the host (MSM_HD).
//
// The textbook schedule, rounds 0-based, for rho < R_F + R_P:
//     s[i] += ark[rho t + i];   s[i] = s[i]^5 for every i (rho < R_F/2 or rho >= R_F/2 + R_P), else for i = 0 only;
//     s'[i] = sum_j mds[i t + j] s[j]
// Every value is a fully reduced residue, so the bytes of a result do not depend on the order of its additions: the body
// adds the constants of round rho + 1 as the first term of the sums of round rho (the constants of round 0 in front of
// the loop), which makes t^2 additions per round and none on a zero.
//
// Code size.  A product is about 400 instructions and the loop of a permutation holds t^2 + 3 t of them as written above:
// more than an instruction cache for t >= 3.  The body therefore takes the S-box and the matrix column by column on s[0]
// and turns the state by one place per step (register moves, 8 t per step against t products): 3 + t products of text.
// No index into the state depends on a loop counter, so the state stays in registers.
//
// Constants image (poseidon_image_records): (R + 1) t records of round constants, R = R_F + R_P, the last t of them zero,
// then the t^2 records of the matrix, row-major; reduced Montgomery residues.
//
// Tree (poseidon_tree_plan).  Arity a = t - 1 >= 2, n_leaves = a^d.  Level k, k < d, holds a^(d-1-k) nodes, level 0 the
// parents of the leaves; node i of a level is the hash of the records a i .. a i + a - 1 of the level below under the
// call's tag.  The inner nodes lie level by level, the root last.  A level of more than 2^TOP nodes is a launch of its
// own; the first level of at most 2^TOP nodes and every level above it run in ONE workgroup that synchronises between
// levels (MSM_AMD_POSEIDON_TOP_LOG).  The root level has one node, so that workgroup always exists.
#pragma once
#include "fr_vec.hip.h"

namespace msm_amd {

constexpr uint32_t kPoseidonMinT = 2, kPoseidonMaxT = 5;
constexpr uint32_t kPoseidonMaxRounds = 128;
constexpr int kPoseidonPermute = 0, kPoseidonHash = 1;
constexpr uint32_t kPoseidonTopLog = 8;       // levels of at most 2^8 nodes share the last workgroup (MSM_AMD_POSEIDON_TOP_LOG)
constexpr uint32_t kPoseidonMaxTopLog = 10;
constexpr uint32_t kPoseidonMaxLevels = 32;   // n_leaves < 2^32 at arity 2

MSM_HD constexpr bool poseidon_shape_ok(uint64_t t, uint64_t r_f, uint64_t r_p) {
  return t >= kPoseidonMinT && t <= kPoseidonMaxT && r_f != 0 && (r_f & 1u) == 0 && r_f <= kPoseidonMaxRounds &&
         r_p <= kPoseidonMaxRounds && r_f + r_p <= kPoseidonMaxRounds;
}
MSM_HD constexpr uint32_t poseidon_ark_records(uint32_t t, uint32_t rounds) { return rounds * t; }
MSM_HD constexpr uint32_t poseidon_mds_at(uint32_t t, uint32_t rounds) { return (rounds + 1) * t; }
MSM_HD constexpr uint32_t poseidon_image_records(uint32_t t, uint32_t rounds) { return (rounds + 1) * t + t * t; }
// products and additions of one textbook permutation
MSM_HD constexpr uint64_t poseidon_products(uint64_t t, uint64_t r_f, uint64_t r_p) { return 3 * (r_f * t + r_p) + (r_f + r_p) * t * t; }
MSM_HD constexpr uint64_t poseidon_additions(uint64_t t, uint64_t r_f, uint64_t r_p) { return (r_f + r_p) * t * t; }

MSM_HD u256 poseidon_sbox(const u256& x) {
  const u256 x2 = Fr::sqr(x);
  return Fr::mul(Fr::sqr(x2), x);
}

template <int T>
MSM_HD void poseidon_turn(u256 (&s)[T]) {
  const u256 first = s[0];
  MSM_UNROLL for (int i = 0; i + 1 < T; ++i) s[i] = s[i + 1];
  s[T - 1] = first;
}

// C: record(i) of the constants image, any i below poseidon_image_records
template <int T, class C>
MSM_HD void poseidon_permute(u256 (&s)[T], const C& c, uint32_t r_f, uint32_t r_p) {
  const uint32_t half = r_f >> 1, rounds = r_f + r_p, mds = poseidon_mds_at(T, rounds);
  MSM_UNROLL for (int i = 0; i < T; ++i) s[i] = Fr::add(s[i], c.record(i));
  NTT_NO_UNROLL for (uint32_t rho = 0; rho < rounds; ++rho) {
    const bool full = rho < half || rho >= half + r_p;
    const uint32_t boxes = full ? (uint32_t)T : 1u;
    NTT_NO_UNROLL for (uint32_t k = 0; k < boxes; ++k) {   // T turns leave the state where it was
      s[0] = poseidon_sbox(s[0]);
      if (full) poseidon_turn<T>(s);
    }
    u256 acc[T];
    MSM_UNROLL for (int i = 0; i < T; ++i) acc[i] = c.record((rho + 1) * T + i);
    NTT_NO_UNROLL for (uint32_t j = 0; j < (uint32_t)T; ++j) {   // column j meets s[j], which stands at s[0]
      MSM_UNROLL for (int i = 0; i < T; ++i) acc[i] = Fr::add(acc[i], Fr::mul(c.record(mds + i * T + j), s[0]));
      poseidon_turn<T>(s);
    }
    MSM_UNROLL for (int i = 0; i < T; ++i) s[i] = acc[i];
  }
}

// ---- the tree: a pure function of the sizes ---------------------------------------------------------------------------------
struct PoseidonTreePlan {
  uint32_t depth;                         // d
  uint32_t arity;
  uint32_t launches;                      // level launches + 1
  uint32_t tail_levels;                   // levels of the last workgroup: depth - (launches - 1)
  uint64_t nodes;                         // (a^d - 1) / (a - 1)
  uint64_t tail_nodes;                    // over the levels of the last workgroup
  uint64_t count[kPoseidonMaxLevels];     // nodes of level k
  uint64_t offset[kPoseidonMaxLevels];    // first record of level k in the tree
};
// n_leaves = arity^d with d >= 1 and arity >= 2: d, else 0
inline uint32_t poseidon_tree_depth(uint64_t n_leaves, uint32_t arity) {
  if (arity < 2 || n_leaves < arity) return 0;
  uint32_t d = 0;
  while (n_leaves > 1) {
    if (n_leaves % arity) return 0;
    n_leaves /= arity, ++d;
  }
  return d;
}
// n_leaves a power of arity, < 2^32; top_log <= kPoseidonMaxTopLog
inline PoseidonTreePlan poseidon_tree_plan(uint64_t n_leaves, uint32_t arity, uint32_t top_log) {
  PoseidonTreePlan p{};
  p.depth = poseidon_tree_depth(n_leaves, arity), p.arity = arity;
  uint64_t count = n_leaves;
  for (uint32_t k = 0; k < p.depth; ++k) {
    count /= arity;
    p.count[k] = count, p.offset[k] = p.nodes;
    p.nodes += count;
    if (count > ((uint64_t)1 << top_log)) ++p.launches;
    else ++p.tail_levels, p.tail_nodes += count;
  }
  ++p.launches;
  return p;
}

}  // namespace msm_amd
