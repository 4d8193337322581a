// The report of the point calls (check, decompress, compress): the 64-byte counters a call's kernels add to, the wave
// routine that adds to them, the same fold for the host twins, and the decode of finished counters into the caller's
// report struct.
// Device: every wave ballots its lanes per reason code and adds the popcounts to the counters with one atomic per wave
// and non-zero counter; the first invalid lane of a wave (the lowest index: lanes are consecutive records) folds
// (index << 3 | reason) into first_key with one 64-bit atomic minimum, so the smallest offending index wins whatever the
// order the workgroups run in.  The optional per-record reason byte is an ordinary store.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace msm_amd {

enum : uint32_t { kPointValid = 0, kPointNotReduced = 1, kPointNotOnCurve = 2, kPointNotInSubgroup = 3, kPointBadEncoding = 4 };

struct PointCounters {
  uint32_t by_reason[5];   // the checks use [0..3]; compress: [1] = records written as all 0xFF
  uint32_t n_identity;
  uint64_t first_key;      // min over invalid records of (index << 3 | reason); all ones = none
  uint32_t pad[8];
};
static_assert(sizeof(PointCounters) == 64 && offsetof(PointCounters, first_key) == 24,
              "PointCounters: 64 bytes, first_key is words 6 and 7 (point_reset_kernel)");

// ---- the fold on the host ------------------------------------------------------------------------------------------
inline PointCounters point_counters_empty() {
  PointCounters c{};
  c.first_key = ~0ull;
  return c;
}
inline void point_counters_add(PointCounters& c, uint64_t index, uint32_t reason, bool identity) {
  ++c.by_reason[reason];
  c.n_identity += identity;
  const uint64_t key = (index << 3) | reason;
  if (reason != kPointValid && key < c.first_key) c.first_key = key;
}
inline void point_counters_merge(PointCounters& sum, const PointCounters& c) {
  for (int k = 0; k < 5; ++k) sum.by_reason[k] += c.by_reason[k];
  sum.n_identity += c.n_identity;
  if (c.first_key < sum.first_key) sum.first_key = c.first_key;
}

// Report: msm_amd_check_report (4 reasons) or msm_amd_decompress_report (5)
template <class Report>
void point_report_decode(const PointCounters& c, size_t n, float device_ms, Report* r) {
  *r = Report{};
  r->n_checked = n;
  for (size_t k = 0; k < sizeof(r->by_reason) / sizeof(r->by_reason[0]); ++k) {
    r->by_reason[k] = c.by_reason[k];
    if (k) r->n_invalid += c.by_reason[k];
  }
  r->n_identity = c.n_identity;
  const bool none = c.first_key == ~0ull;
  r->first_invalid = none ? UINT64_MAX : (c.first_key >> 3);
  r->first_reason = none ? 0u : (uint32_t)(c.first_key & 7u);
  r->device_ms = device_ms;
}

// ---- the fold on the device ----------------------------------------------------------------------------------------
#if defined(__HIPCC__)
// NR: reason codes the kernel can produce (4: the checks, 5: decompression), one ballot each
template <uint32_t NR>
__device__ __forceinline__ void point_report(bool active, uint32_t t, uint32_t reason, bool identity,
                                             uint8_t* __restrict__ reasons, PointCounters* __restrict__ counters) {
  if (active && reasons) reasons[t] = (uint8_t)reason;
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t r = 0; r < NR; ++r) {
    const uint64_t m = __ballot(active && reason == r);
    if (lane == 0 && m) atomicAdd(&counters->by_reason[r], (uint32_t)__popcll(m));
  }
  const uint64_t mi = __ballot(active && identity);
  if (lane == 0 && mi) atomicAdd(&counters->n_identity, (uint32_t)__popcll(mi));
  const uint64_t bad = __ballot(active && reason != kPointValid);
  if (bad && lane == (uint32_t)(__ffsll((unsigned long long)bad) - 1))
    atomicMin(reinterpret_cast<unsigned long long*>(&counters->first_key), ((unsigned long long)t << 3) | reason);
}
#endif

}  // namespace msm_amd
