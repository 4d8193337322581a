// Multilinear tables over BN254 Fr and the rounds of a sumcheck (msm_amd_fr_mle_bind*, msm_amd_fr_mle_eval*,
// msm_amd_fr_eq_table*, msm_amd_fr_sumcheck_round*): the bodies shared by the kernels (k_fr.hip), the host twins
// (host_fr.hip) and the host driver (msm_host.hip).  Everything here compiles for the device and for the host (MSM_HD).
//
// A table is n = 2^m records f[i], the value at x_j = bit j of i.  One step folds one variable at a challenge r:
//   LOW   binds the lowest variable left:  f'[i] = fold(f[2i], f[2i + 1], r)
//   HIGH  binds the highest variable left: f'[i] = fold(f[i], f[i + n/2], r)
// with fold(lo, hi, r) = lo + r (hi - lo): one product.  Folds of different variables commute, so a kernel may take the
// variables of one launch in the order that suits its loads, as long as every variable meets its own challenge.
//
// Round (fr_mle_round_plan).  h = n/2 pairs; one wave per chunk of 2^C consecutive pairs (MSM_AMD_FR_MLE_CHUNK_LOG), d + 1
// raw partial records per wave, plane t of a level holding the partials of g(t) side by side.  One wave: the partials are
// the values.  More: fold launches of one wave per 2^kFrMleFoldLog partials of one t, until one record per t is left.
// Every level has its own records, so that no launch reads what a workgroup of the same launch wrote.
//
// Eval (fr_scan_plan).  A tile of 2^T records of one table folds to one record: level k + 1 holds one record per tile of
// level k, the last level one record per table.  Level k binds the variables T k .. of LOW (HIGH: the point reversed).
//
// Bind (fr_mle_bind_plan).  A launch folds up to kFrMleBindVars variables while the 2^k records of an output pass through
// registers.  HIGH works in place from the second launch on; LOW alternates between the output and ctx-owned memory so
// that the last launch writes the output.
#pragma once
#include "fr_vec.hip.h"

namespace msm_amd {

constexpr int kFrMleLow = 0, kFrMleHigh = 1;
constexpr int kFrSumProduct = 0, kFrSumEqAbC = 1;
constexpr uint32_t kFrMleMaxTables = 4;
constexpr uint32_t kFrMleMaxValues = kFrMleMaxTables + 1;   // d + 1
constexpr uint32_t kFrMleChunkLog = 8;      // pairs per wave of a round, as a power of two (MSM_AMD_FR_MLE_CHUNK_LOG)
constexpr uint32_t kFrMleMinChunkLog = 6, kFrMleMaxChunkLog = 20;
constexpr uint32_t kFrMleFoldLog = 10;      // partials of one t per wave of a fold launch
constexpr uint32_t kFrMleBindVars = 3;      // variables per bind launch: eight records per output
constexpr uint32_t kFrMleMaxVars = 31;
constexpr uint32_t kFrMleEqSpread = 3;      // eq table: a lane of the wide kernel writes 2^3 outputs
constexpr uint32_t kFrMleEqWideFrom = 9;    // m from which the wide kernel runs: 64 lanes and more
constexpr uint32_t kFrMleMaxFoldLevels = 4; // 2^25 waves at the smallest chunk / 2^10 per level

MSM_HD constexpr bool fr_mle_order_known(int order) { return order == kFrMleLow || order == kFrMleHigh; }
// the degree d of a round's polynomial; 0: the form does not take this many tables
MSM_HD constexpr uint32_t fr_mle_degree(int form, uint64_t n_vec) {
  return form == kFrSumProduct ? (n_vec >= 1 && n_vec <= kFrMleMaxTables ? (uint32_t)n_vec : 0u)
         : form == kFrSumEqAbC ? (n_vec == 4 ? 3u : 0u)
                               : 0u;
}
MSM_HD constexpr uint32_t fr_mle_log2(uint64_t n) {
  uint32_t m = 0;
  while (((uint64_t)1 << (m + 1)) <= n) ++m;
  return m;
}

// one step at one output
MSM_HD u256 fr_mle_fold(const u256& lo, const u256& hi, const u256& r) { return Fr::add(lo, Fr::mul(r, Fr::sub(hi, lo))); }

// The d + 1 running sums of a round, in registers: every index below is a constant after unrolling.
template <int FORM, int K>
struct FrMleSums {
  static constexpr int kValues = FORM == kFrSumProduct ? K + 1 : 4;
  u256 g[kValues];
  MSM_HD void clear() {
    MSM_UNROLL for (int t = 0; t < kValues; ++t) g[t] = u256_zero();
  }
  // F at t = 0 .. d for one pair of every table.  f_j(0) = lo_j, and every operand advances from t to t + 1 by its
  // difference: one addition, no product by t.  Only f and the differences stay in registers.  PRODUCT of K tables: K - 1
  // products per t; EQ_AB_C: two.
  MSM_HD void add_pair(const u256 (&lo)[K], const u256 (&hi)[K]) {
    u256 f[K], diff[K];
    MSM_UNROLL for (int j = 0; j < K; ++j) f[j] = lo[j], diff[j] = Fr::sub(hi[j], lo[j]);
    MSM_UNROLL for (int t = 0; t < kValues; ++t) {
      if (t > 0) {
        MSM_UNROLL for (int j = 0; j < K; ++j) f[j] = Fr::add(f[j], diff[j]);
      }
      u256 v;
      if (FORM == kFrSumProduct) {
        v = f[0];
        MSM_UNROLL for (int j = 1; j < K; ++j) v = Fr::mul(v, f[j]);
      } else {
        v = Fr::mul(f[0], Fr::sub(Fr::mul(f[1 % K], f[2 % K]), f[3 % K]));
      }
      g[t] = Fr::add(g[t], v);
    }
  }
};

// ---- a round over a caller's sum of products (msm_amd_fr_sumcheck_round_terms*, msm_amd_fr_sumcheck_step_terms*) ---------
// F = [f_outer] sum_k c_k prod_j f_(idx[k][j]).  The image of a checked term list is plain data and travels by value (664
// bytes): reduced Montgomery coefficients, and the lengths, the kinds and the table indices as bytes packed into words, so
// that a kernel reads them with scalar loads at wave-uniform offsets.
constexpr uint32_t kFrSumMaxTables = 16, kFrSumMaxTerms = 16, kFrSumMaxFactors = 6;
constexpr uint32_t kFrSumMaxValues = kFrSumMaxFactors + 2;   // d + 1 with an outer factor
constexpr uint32_t kFrSumNoOuter = 0xFFFFFFFFu;
constexpr uint32_t kFrCoeffAny = 0, kFrCoeffOne = 1, kFrCoeffMinusOne = 2;   // 1 and r - 1 cost no product
struct FrSumTerms {
  u256 coeff[kFrSumMaxTerms];
  uint32_t n_terms, outer;
  uint32_t len[kFrSumMaxTerms / 4], kind[kFrSumMaxTerms / 4];
  uint32_t idx[kFrSumMaxTerms * kFrSumMaxFactors / 4];
};
MSM_HD uint32_t fr_sum_byte(const uint32_t* words, uint32_t i) { return (words[i >> 2] >> ((i & 3u) * 8u)) & 0xFFu; }
inline void fr_sum_set_byte(uint32_t* words, uint32_t i, uint32_t b) { words[i >> 2] |= b << ((i & 3u) * 8u); }
// the degree d of the round's polynomial
inline uint32_t fr_sum_degree(const FrSumTerms& s) {
  uint32_t longest = 0;
  for (uint32_t k = 0; k < s.n_terms; ++k) longest = fr_sum_byte(s.len, k) > longest ? fr_sum_byte(s.len, k) : longest;
  return longest + (s.outer != kFrSumNoOuter ? 1u : 0u);
}
// The V = d + 1 running sums of such a round.  Terms outermost, so that a pair of a table is loaded once per use: the first
// factor of a term gives p[t] = c_k f(t) (the coefficient goes into f and its difference: two products, none for 1 and
// r - 1, which is subtracted), every further factor multiplies p[t] by its f(t), every operand advancing from t to t + 1 by
// its difference; acc[t] collects the terms of the pair and meets the outer factor once per t.  Live across a factor: the V
// sums, acc and p.  Beyond four values that does not fit 256 registers, so the values are taken in passes of W (3, or 2 of 8) at a time
// (fr_sum_pass): a pass walks the terms for t = T0 .. T0 + W - 1, its operands starting at f(T0) = lo + T0 diff (additions).
// The loops over terms and factors are runtime loops with the same trip counts in every lane; the t loops are unrolled and
// no array is indexed at run time.  load(table, lo, hi) brings the two records of a pair.  Field arithmetic is exact: any
// order gives these bytes.
MSM_HD constexpr int fr_sum_pass(int values) { return values <= 4 ? values : values <= 7 ? 3 : 2; }
template <int V>
struct FrTermSums {
  static constexpr int kPass = fr_sum_pass(V);
  u256 g[V];
  MSM_HD void clear() {
    MSM_UNROLL for (int t = 0; t < V; ++t) g[t] = u256_zero();
  }
  // f(T0) and the difference of one operand
  template <int T0>
  static MSM_HD void operand(const u256& lo, const u256& hi, u256& f, u256& diff) {
    f = lo, diff = Fr::sub(hi, lo);
    MSM_UNROLL for (int t = 0; t < T0; ++t) f = Fr::add(f, diff);
  }
  template <int T0, int W, class Load>
  MSM_HD void pass(const FrSumTerms& s, Load&& load) {
    u256 acc[W], lo, hi, f, diff;
    MSM_UNROLL for (int t = 0; t < W; ++t) acc[t] = u256_zero();
    uint32_t at = 0;
    NTT_NO_UNROLL for (uint32_t k = 0; k < s.n_terms; ++k) {
      const uint32_t len = fr_sum_byte(s.len, k), kind = fr_sum_byte(s.kind, k);
      u256 p[W];
      load(fr_sum_byte(s.idx, at), lo, hi);
      operand<T0>(lo, hi, f, diff);
      if (kind == kFrCoeffAny) f = Fr::mul(s.coeff[k], f), diff = Fr::mul(s.coeff[k], diff);
      MSM_UNROLL for (int t = 0; t < W; ++t) {
        if (t > 0) f = Fr::add(f, diff);
        p[t] = f;
      }
      NTT_NO_UNROLL for (uint32_t j = 1; j < len; ++j) {
        load(fr_sum_byte(s.idx, at + j), lo, hi);
        operand<T0>(lo, hi, f, diff);
        MSM_UNROLL for (int t = 0; t < W; ++t) {
          if (t > 0) f = Fr::add(f, diff);
          p[t] = Fr::mul(p[t], f);
        }
      }
      if (kind == kFrCoeffMinusOne) {
        MSM_UNROLL for (int t = 0; t < W; ++t) acc[t] = Fr::sub(acc[t], p[t]);
      } else {
        MSM_UNROLL for (int t = 0; t < W; ++t) acc[t] = Fr::add(acc[t], p[t]);
      }
      at += len;
    }
    if (s.outer != kFrSumNoOuter) {
      load(s.outer, lo, hi);
      operand<T0>(lo, hi, f, diff);
      MSM_UNROLL for (int t = 0; t < W; ++t) {
        if (t > 0) f = Fr::add(f, diff);
        g[T0 + t] = Fr::add(g[T0 + t], Fr::mul(f, acc[t]));
      }
    } else {
      MSM_UNROLL for (int t = 0; t < W; ++t) g[T0 + t] = Fr::add(g[T0 + t], acc[t]);
    }
  }
  template <int T0, class Load>
  MSM_HD void passes_from(const FrSumTerms& s, Load&& load) {
    if constexpr (T0 < V) {
      pass<T0, (V - T0 < kPass ? V - T0 : kPass)>(s, load);
      passes_from<T0 + kPass>(s, load);
    }
  }
  template <class Load>
  MSM_HD void add_pair(const FrSumTerms& s, Load&& load) { passes_from<0>(s, load); }
};

// products per pair of that order: (len_k - 1) V per term, V for the outer factor, and per pass two for every coefficient
// that is neither 1 nor r - 1
inline uint64_t fr_sum_products(const FrSumTerms& s) {
  const uint64_t values = fr_sum_degree(s) + 1, pass = fr_sum_pass((int)values), passes = (values + pass - 1) / pass;
  uint64_t c = s.outer != kFrSumNoOuter ? values : 0;
  for (uint32_t k = 0; k < s.n_terms; ++k)
    c += (fr_sum_byte(s.len, k) - 1) * values + (fr_sum_byte(s.kind, k) == kFrCoeffAny ? 2u * passes : 0u);
  return c;
}

// ---- plans: pure functions of the sizes ----------------------------------------------------------------------------------
struct FrMleRoundPlan {
  uint32_t values;                          // d + 1
  uint32_t chunk_log;                       // pairs per wave, as a power of two: min(C, log2 h)
  uint32_t levels;                          // 1 + fold launches
  uint32_t launches;
  uint64_t count[kFrMleMaxFoldLevels + 1];  // partials per t that level k leaves; count[levels - 1] = 1
  uint64_t offset[kFrMleMaxFoldLevels + 1]; // first record of level k in the workspace
  uint64_t waves;                           // dispatched over all launches
  uint64_t records;                         // the workspace
  uint64_t values_off;                      // first record of the d + 1 values: offset[levels - 1]
};
// n a power of two >= 2, d + 1 values, chunk_log: kFrMleMinChunkLog .. kFrMleMaxChunkLog
inline FrMleRoundPlan fr_mle_round_plan(uint64_t n, uint32_t values, uint32_t chunk_log) {
  FrMleRoundPlan p{};
  const uint32_t h_log = fr_mle_log2(n) - 1;
  p.values = values;
  p.chunk_log = chunk_log < h_log ? chunk_log : h_log;
  uint64_t count = (uint64_t)1 << (h_log - p.chunk_log);
  p.waves = count;
  for (;;) {
    p.count[p.levels] = count, p.offset[p.levels] = p.records;
    p.records += count * values;
    ++p.levels;
    if (count == 1) break;
    count = (count + ((uint64_t)1 << kFrMleFoldLog) - 1) >> kFrMleFoldLog;
    p.waves += count * values;
  }
  p.launches = p.levels;
  p.values_off = p.offset[p.levels - 1];
  return p;
}

struct FrMleBindPlan {
  uint32_t launches;
  uint32_t vars[kFrMleMaxVars];            // variables of launch k
  uint64_t work_records;                    // LOW with more than one launch: the records the launches alternate through
  uint64_t waves;
};
// n_bind: 1 .. log2 n.  The launches take kFrMleBindVars variables each, the last one what is left.
inline FrMleBindPlan fr_mle_bind_plan(int order, uint64_t n, uint64_t n_vec, uint32_t n_bind) {
  FrMleBindPlan p{};
  uint64_t len = n;
  for (uint32_t left = n_bind; left != 0;) {
    const uint32_t k = left < kFrMleBindVars ? left : kFrMleBindVars;
    p.vars[p.launches++] = k;
    left -= k, len >>= k;
    p.waves += (len * n_vec + kFrWave - 1) / kFrWave;
  }
  if (order == kFrMleLow && p.launches > 1) p.work_records = (n >> p.vars[0]) * n_vec;
  return p;
}

// records per lane of an eval tile of cnt = 2^c records, as a power of two
MSM_HD constexpr uint32_t fr_mle_per_log(uint64_t cnt) { return cnt > kFrWave ? fr_mle_log2(cnt) - 6u : 0u; }

}  // namespace msm_amd
