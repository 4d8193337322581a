// Host twin of the sort of Fr records by canonical value (fr_sort.hip.h; no ctx, no GPU), the argument check it shares with
// the host driver (calls_fr.hip), and the planner aid.  The twin does not sort by digits: the keys of every record are formed
// first (out may be the inputs), then every column is a stable merge sort of its indices by fr_sort_less -- ranges sorted by the
// host threads, then merged pairwise -- so that it shares nothing with the kernels but the key.  A stable sort has one
// answer, so neither the thread count nor the way the ranges are cut shows in any byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_fr.h"

namespace msm_amd {

const char* fr_sort_call_check(int mem, int scalar_layout, const void* in, uint64_t n, uint64_t n_vec, const void* out,
                               const uint32_t* perm_out) {
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE) return "mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE";
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (!out && !perm_out) return "out or perm_out must be given";
  if (n == 0 || n_vec == 0) return nullptr;
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (!in) return "null pointer with n > 0";
  const bool device = mem == MSM_AMD_MEM_DEVICE;
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return "device records must be 16-byte aligned";
  if (device && ((uintptr_t)perm_out & 3u)) return "device perm_out must be 4-byte aligned";
  const uint64_t bytes = n * n_vec * 32, perm_bytes = n * n_vec * 4;
  const uintptr_t f = (uintptr_t)in, o = (uintptr_t)out, p = (uintptr_t)perm_out;
  if (out && o != f && o < f + bytes && f < o + bytes) return "out must be the inputs themselves or not overlap them";
  if (perm_out && p < f + bytes && f < p + perm_bytes) return "perm_out must not overlap the inputs";
  if (perm_out && out && p < o + bytes && o < p + perm_bytes) return "perm_out must not overlap out";
  return nullptr;
}

int host_fr_sort(int layout, const void* in_v, size_t n, size_t n_vec, int threads, void* out_v, uint32_t* perm_out) {
  if (fr_sort_call_check(MSM_AMD_MEM_HOST, layout, in_v, n, n_vec, out_v, perm_out)) return MSM_AMD_INPUT_ERROR;
  const size_t total = n * n_vec;
  if (total == 0) return MSM_AMD_OK;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  std::vector<u256> keys(total);
  for_ranges(worker_count(threads, total), total, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      u256 rec;
      std::memcpy(rec.v, in + i * 32, 32);
      keys[i] = fr_sort_key(layout, rec);
    }
  });
  std::vector<uint32_t> perm(n);
  const unsigned T = worker_count(threads, n);
  const size_t chunk = (n + T - 1) / T;   // the ranges of for_ranges
  for (size_t v = 0; v < n_vec; ++v) {
    const u256* key = keys.data() + v * n;
    auto less = [&](uint32_t a, uint32_t b) { return fr_sort_less(key[a], key[b]); };
    for_ranges(T, n, [&](unsigned, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) perm[i] = (uint32_t)i;
      std::stable_sort(perm.begin() + lo, perm.begin() + hi, less);
    });
    // sorted runs of `run` ranges are merged two by two; the pairs of one round are disjoint and run on threads of their own
    for (size_t run = 1; run < T; run *= 2) {
      const size_t pairs = (T + 2 * run - 1) / (2 * run);
      for_ranges((unsigned)pairs, pairs, [&](unsigned, size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; ++k) {
          const size_t first = std::min(n, 2 * k * run * chunk), mid = std::min(n, first + run * chunk);
          const size_t last = std::min(n, mid + run * chunk);
          std::inplace_merge(perm.begin() + first, perm.begin() + mid, perm.begin() + last, less);
        }
      });
    }
    for_ranges(T, n, [&](unsigned, size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        if (out) {
          const u256 rec = fr_sort_record(layout, key[perm[k]]);
          std::memcpy(out + (v * n + k) * 32, rec.v, 32);
        }
        if (perm_out) perm_out[v * n + k] = perm[k];
      }
    });
  }
  return MSM_AMD_OK;
}

}  // namespace msm_amd

extern "C" {

int msm_amd_host_fr_sort(int scalar_layout, const void* in, size_t n, size_t n_vec, int threads, void* out, uint32_t* perm_out) {
  return msm_amd::host_fr_sort(scalar_layout, in, n, n_vec, threads, out, perm_out);
}

int msm_amd_test_fr_sort_plan(size_t n, size_t n_vec, uint32_t digit_mask, uint64_t out[4]) {
  if (n == 0 || n_vec == 0 || ((uint64_t)n >> 32) || ((uint64_t)n_vec >> 32) || (((uint64_t)n * n_vec) >> 32) || !out)
    return MSM_AMD_INPUT_ERROR;
  const msm_amd::FrSortPlan p = msm_amd::fr_sort_plan(n, n_vec, digit_mask);
  out[0] = p.passes, out[1] = p.launches, out[2] = p.tiles, out[3] = p.bytes;
  return MSM_AMD_OK;
}

}  // extern "C"
