// Host twin of the transform (no ctx, no GPU): the butterfly, conversion and scaling bodies of ntt.hip.h on the CPU, one
// level of the network at a time, each level split over the host threads; the argument checks the twin shares with
// the host driver (msm_host.hip); and the test aids that need no ctx: the twin stopped after some levels, the plan and
// the slot map of ntt.hip.h as the kernels see them.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_ntt.h"

namespace msm_amd {

static_assert(kNttRootArk == MSM_AMD_NTT_ROOT_ARK && kNttRootH2c == MSM_AMD_NTT_ROOT_H2C, "roots");
static_assert(kNttForward == MSM_AMD_NTT_FORWARD && kNttInverse == MSM_AMD_NTT_INVERSE, "directions");
static_assert(kNttMontLe == MSM_AMD_SCALAR_MONT_LE && kNttCanonLe == MSM_AMD_SCALAR_CANON_LE, "scalar layouts as ntt_load reads them");
static_assert(sizeof(u256) == 32, "records");

bool ntt_root_known(int root) { return root == kNttRootArk || root == kNttRootH2c; }
bool ntt_direction_known(int direction) { return direction == kNttForward || direction == kNttInverse; }
bool ntt_layout_known(int scalar_layout) { return scalar_layout == kNttMontLe || scalar_layout == kNttCanonLe; }

bool ntt_read_shift(int scalar_layout, const void* shift32, u256* g) {
  if (!shift32) {
    *g = Fr::one();
    return true;
  }
  uint32_t rec[8];
  std::memcpy(rec, shift32, 32);
  *g = ntt_load(scalar_layout, rec);
  return !u256_is_zero(*g);
}

namespace {

constexpr uint32_t kAllLevels = ~0u;

// levels == kAllLevels: the transform.  levels <= log_n (msm_amd_test_host_ntt_levels): the work array after that many
// levels as it stands -- Montgomery residues at the positions of the network, no permutation, no scaling.
int host_ntt(int root, uint32_t log_n, int direction, int layout, const void* shift32, const void* in_v, void* out_v,
             size_t n_vec, int threads, uint32_t levels) {
  if (!ntt_root_known(root) || !ntt_direction_known(direction) || !ntt_layout_known(layout) || log_n > kNttMaxLog ||
      ((uint64_t)n_vec >> (32 - log_n)) != 0 || (levels != kAllLevels && levels > log_n))
    return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  u256 g;
  if (!in_v || !out_v || !ntt_read_shift(layout, shift32, &g)) return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const size_t n = (size_t)1 << log_n, total = n_vec << log_n;
  const uint32_t nmask = (uint32_t)(n - 1);
  const bool inverse = direction == kNttInverse, shift = shift32 != nullptr;
  u256 tab[kNttPowEntries];
  NttScale sc;
  ntt_shift_setup(g, direction, log_n, tab, &sc);

  // w^j, j < n/2: every range starts from a power and steps by w
  const u256 omega = ntt_omega(root, log_n);
  std::vector<u256> tw(n / 2);
  if (!tw.empty()) {
    u256 wtab[kNttPowEntries];
    ntt_pow_table(omega, wtab);
    for_ranges(worker_count(threads, tw.size()), tw.size(), [&](unsigned, size_t lo, size_t hi) {
      if (lo >= hi) return;
      u256 w = ntt_pow(wtab, (uint32_t)lo);
      for (size_t j = lo; j < hi; ++j) {
        tw[j] = w;
        w = Fr::mul(w, omega);
      }
    });
  }

  std::vector<u256> work(total);
  const unsigned T = worker_count(threads, total);
  for_ranges(T, total, [&](unsigned, size_t lo, size_t hi) {
    for (size_t idx = lo; idx < hi; ++idx) {
      uint32_t rec[8];
      std::memcpy(rec, in + idx * 32, 32);
      u256 x = ntt_load(layout, rec);
      if (shift && !inverse) x = Fr::mul(x, ntt_pow(tab, (uint32_t)idx & nmask));
      work[idx] = x;
    }
  });
  for (uint32_t level = 0; level < (levels == kAllLevels ? log_n : levels); ++level) {
    const uint32_t bit = log_n - 1 - level;
    const size_t h = (size_t)1 << bit;
    for_ranges(worker_count(threads, total / 2), total / 2, [&](unsigned, size_t lo, size_t hi) {
      for (size_t f = lo; f < hi; ++f) {
        const size_t idx = ((f >> bit) << (bit + 1)) | (f & (h - 1));
        ntt_bfly(work[idx], work[idx + h], tw[ntt_twiddle_index((uint32_t)idx & nmask, log_n, level)]);
      }
    });
  }
  if (levels != kAllLevels) {
    std::memcpy(out, work.data(), total * 32);
    return MSM_AMD_OK;
  }
  for_ranges(T, total, [&](unsigned, size_t lo, size_t hi) {
    for (size_t idx = lo; idx < hi; ++idx) {
      const uint32_t i = (uint32_t)idx & nmask, k = ntt_bitrev(i, log_n);   // position i holds X[k]
      u256 x = work[idx];
      if (inverse) x = Fr::mul(x, shift && k != 0 ? Fr::mul(sc.c0, ntt_pow(tab, k)) : sc.c1);
      const uint32_t j = inverse ? (uint32_t)((n - k) & nmask) : k;
      uint32_t rec[8];
      ntt_store(layout, x, rec);
      std::memcpy(out + ((idx - i) + j) * 32, rec, 32);
    }
  });
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_host_ntt(int root, uint32_t log_n, int direction, int scalar_layout, const void* shift32, const void* in,
                     void* out, size_t n_vec, int threads) {
  return msm_amd::host_ntt(root, log_n, direction, scalar_layout, shift32, in, out, n_vec, threads, msm_amd::kAllLevels);
}

int msm_amd_test_host_ntt_levels(int root, uint32_t log_n, int direction, int scalar_layout, const void* shift32,
                                 const void* in, void* out, size_t n_vec, uint32_t levels, int threads) {
  if (levels == msm_amd::kAllLevels) return MSM_AMD_INPUT_ERROR;
  return msm_amd::host_ntt(root, log_n, direction, scalar_layout, shift32, in, out, n_vec, threads, levels);
}

int msm_amd_test_ntt_plan(uint32_t log_n, uint32_t tile_log, uint32_t* out) {
  using namespace msm_amd;
  if (!out || log_n > kNttMaxLog || tile_log < 2 || tile_log > kNttTileLog) return MSM_AMD_INPUT_ERROR;
  const NttPlan plan = ntt_plan(log_n, tile_log);
  out[0] = plan.passes;
  uint32_t level = 0;
  for (uint32_t k = 0; k < plan.passes; ++k) {
    const NttPass p = ntt_pass(log_n, level, plan.levels[k], tile_log);
    out[1 + 4 * k] = p.level0, out[2 + 4 * k] = p.levels, out[3 + 4 * k] = p.sigma, out[4 + 4 * k] = p.low;
    level += plan.levels[k];
  }
  return MSM_AMD_OK;
}

int msm_amd_test_ntt_slots(uint32_t log_n, uint32_t tile_log, uint32_t pass, uint64_t wg, uint64_t* out) {
  using namespace msm_amd;
  if (!out || log_n > kNttMaxLog || tile_log < 2 || tile_log > kNttTileLog || (wg >> 32) != 0) return MSM_AMD_INPUT_ERROR;
  const NttPlan plan = ntt_plan(log_n, tile_log);
  if (pass >= plan.passes) return MSM_AMD_INPUT_ERROR;
  uint32_t level = 0;
  for (uint32_t k = 0; k < pass; ++k) level += plan.levels[k];
  const NttPass p = ntt_pass(log_n, level, plan.levels[pass], tile_log);
  for (uint32_t m = 0; m < (1u << tile_log); ++m) out[m] = ntt_slot_index(p, wg, m);
  return MSM_AMD_OK;
}

}  // extern "C"
