// Point validation kernels: judge the records of a caller's point array instead of summing them (check_points.hip.h).
//   check_g1_kernel   one lane per G1 record in the caller's layout: range, curve equation
//   check_g2_kernel   one lane per G2 record: range, curve equation over Fq2, and on request the subgroup rule
//                     (the endomorphism identity; a 63-bit double-and-add per record)
// Report: every wave ballots its lanes per reason code and adds the popcounts to the 64-byte CheckCounters with one
// atomic per wave and counter; the first invalid lane of a wave (the lowest index: lanes are consecutive records) folds
// (index << 2 | reason) into first_key with one 64-bit atomic minimum, so the smallest offending index wins whatever the
// order the workgroups run in.  The optional per-record reason byte is an ordinary store.
// None of these kernels uses scratch (`make resource-usage`, tests/test_check_host.py).
#include "launch_check.h"

namespace msm_amd {

__device__ __forceinline__ void check_report(bool active, uint32_t t, uint32_t reason, bool identity,
                                             uint8_t* __restrict__ reasons, CheckCounters* __restrict__ counters) {
  if (active && reasons) reasons[t] = (uint8_t)reason;
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    const uint64_t m = __ballot(active && reason == r);
    if (lane == 0 && m) atomicAdd(&counters->by_reason[r], (uint32_t)__popcll(m));
  }
  const uint64_t mi = __ballot(active && identity);
  if (lane == 0 && mi) atomicAdd(&counters->n_identity, (uint32_t)__popcll(mi));
  const uint64_t bad = __ballot(active && reason != kPointValid);
  if (bad && lane == (uint32_t)(__ffsll((unsigned long long)bad) - 1))
    atomicMin(reinterpret_cast<unsigned long long*>(&counters->first_key), ((unsigned long long)t << 2) | reason);
}

__global__ void __launch_bounds__(64) check_reset_kernel(CheckCounters* __restrict__ counters) {
  uint32_t* w = reinterpret_cast<uint32_t*>(counters);
  if (threadIdx.x < 16) w[threadIdx.x] = (threadIdx.x == 6 || threadIdx.x == 7) ? 0xFFFFFFFFu : 0u;
}
static_assert(offsetof(CheckCounters, first_key) == 24, "check_reset_kernel writes first_key as words 6, 7");

__global__ void __launch_bounds__(256)
check_g1_kernel(const uint8_t* __restrict__ in, int layout, uint32_t stride, uint32_t n, uint8_t* __restrict__ reasons,
                CheckCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) reason = check_record_g1(layout, in + (size_t)t * stride, identity);
  check_report(active, t, reason, identity, reasons, counters);
}

__global__ void __launch_bounds__(64)
check_g2_kernel(const uint8_t* __restrict__ in, int ark, uint32_t n, uint32_t checks, uint8_t* __restrict__ reasons,
                CheckCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) reason = check_record_g2(ark, in + (size_t)t * (ark ? 136 : 128), checks, identity);
  check_report(active, t, reason, identity, reasons, counters);
}

void launch_check_reset(hipStream_t st, CheckCounters* counters) {
  hipLaunchKernelGGL(check_reset_kernel, dim3(1), dim3(64), 0, st, counters);
}

void launch_check_g1(hipStream_t st, const void* in, int layout, uint32_t stride, uint32_t n, uint8_t* reasons,
                     CheckCounters* counters) {
  hipLaunchKernelGGL(check_g1_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, (const uint8_t*)in, layout, stride, n,
                     reasons, counters);
}

void launch_check_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t checks, uint8_t* reasons,
                     CheckCounters* counters) {
  hipLaunchKernelGGL(check_g2_kernel, dim3((uint32_t)(((uint64_t)n + 63) / 64)), dim3(64), 0, st, (const uint8_t*)in, ark, n, checks, reasons,
                     counters);
}

}  // namespace msm_amd
