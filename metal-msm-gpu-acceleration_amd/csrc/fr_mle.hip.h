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
