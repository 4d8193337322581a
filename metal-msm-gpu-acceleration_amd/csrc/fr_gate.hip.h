// Gate polynomials over rotated Fr columns (msm_amd_fr_gate_eval, msm_amd_host_fr_gate_eval): the body shared by the kernel
// (k_fr.hip) and the host twin (host_fr.hip).  Everything here compiles for the device and for the host (MSM_HD).
//
// n_vec columns of n records; for every row i
//   v[i] = sum_k c_k prod_j col_(idx[k][j])[(i + off[slot[k][j]]) mod n]
// where off holds the at most 8 distinct values (rot rot_step) mod n of the call, reduced on the host: a row is one
// addition and one conditional subtraction, nothing is reduced mod n per lane.  The image of a checked term list is plain
// data and travels by value (840 bytes), as FrSumTerms (fr_mle.hip.h): reduced Montgomery coefficients, and the lengths, the
// kinds, the column indices and the offset slots as bytes packed into words, read at wave-uniform offsets.
#pragma once
#include "fr_mle.hip.h"

namespace msm_amd {

constexpr uint32_t kFrGateMaxTerms = 16, kFrGateMaxFactors = 8, kFrGateMaxOffsets = 8, kFrGateMaxCols = 256;
constexpr uint32_t kFrGateMaxPeriod = 256;
constexpr uint32_t kFrGateAccumulate = 1;   // flags
struct FrGateTerms {
  u256 coeff[kFrGateMaxTerms];
  uint32_t n_terms, n_offsets;
  uint32_t offset[kFrGateMaxOffsets];   // each below n
  uint32_t len[kFrGateMaxTerms / 4], kind[kFrGateMaxTerms / 4];   // kind: kFrCoeffAny, kFrCoeffOne, kFrCoeffMinusOne
  uint32_t col[kFrGateMaxTerms * kFrGateMaxFactors / 4], slot[kFrGateMaxTerms * kFrGateMaxFactors / 4];
};

// the row a factor reads: i < n and offset < n < 2^32
MSM_HD uint64_t fr_gate_at(const FrGateTerms& g, uint32_t factor, uint64_t i, uint64_t n) {
  const uint64_t r = i + g.offset[fr_sum_byte(g.slot, factor)];
  return r >= n ? r - n : r;
}

// v[i].  Terms outermost, factors inside: runtime loops with the same trip counts in every lane.  Live across a load: the
// row's sum, the running product and the operand; no array is indexed at run time.  load(column, row) brings one record
// as a reduced Montgomery residue.  A coefficient of 1 or r - 1 costs no product (r - 1 is subtracted); field arithmetic
// is exact, so any order gives these bytes.
template <class Load>
MSM_HD u256 fr_gate_row(const FrGateTerms& g, uint64_t i, uint64_t n, Load&& load) {
  u256 sum = u256_zero();
  uint32_t at = 0;
  NTT_NO_UNROLL for (uint32_t k = 0; k < g.n_terms; ++k) {
    const uint32_t len = fr_sum_byte(g.len, k), kind = fr_sum_byte(g.kind, k);
    u256 p = load(fr_sum_byte(g.col, at), fr_gate_at(g, at, i, n));
    NTT_NO_UNROLL for (uint32_t j = 1; j < len; ++j) p = Fr::mul(p, load(fr_sum_byte(g.col, at + j), fr_gate_at(g, at + j, i, n)));
    if (kind == kFrCoeffAny) p = Fr::mul(g.coeff[k], p);
    if (kind == kFrCoeffMinusOne) sum = Fr::sub(sum, p);
    else sum = Fr::add(sum, p);
    at += len;
  }
  return sum;
}

// products per row of that order: (len - 1) per term, one for a coefficient that is neither 1 nor r - 1
inline uint64_t fr_gate_products(const FrGateTerms& g) {
  uint64_t c = 0;
  for (uint32_t k = 0; k < g.n_terms; ++k) c += fr_sum_byte(g.len, k) - 1 + (fr_sum_byte(g.kind, k) == kFrCoeffAny ? 1u : 0u);
  return c;
}
inline uint64_t fr_gate_factors(const FrGateTerms& g) {
  uint64_t c = 0;
  for (uint32_t k = 0; k < g.n_terms; ++k) c += fr_sum_byte(g.len, k);
  return c;
}
inline uint32_t fr_gate_degree(const FrGateTerms& g) {
  uint32_t d = 0;
  for (uint32_t k = 0; k < g.n_terms; ++k) d = fr_sum_byte(g.len, k) > d ? fr_sum_byte(g.len, k) : d;
  return d;
}

}  // namespace msm_amd
