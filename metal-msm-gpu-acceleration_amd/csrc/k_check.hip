// Point validation kernels: judge the records of a caller's point array instead of summing them (check_points.hip.h).
//   check_g1_kernel   one lane per G1 record in the caller's layout: range, curve equation
//   check_g2_kernel   one lane per G2 record: range, curve equation over Fq2, and on request the subgroup rule
//                     (the endomorphism identity; a 63-bit double-and-add per record)
//   point_reset_kernel   the 64-byte PointCounters of a check, decompress or compress call: zero, first_key all ones
// Report: point_report<4> of point_report.hip.h.
// None of these kernels uses scratch (`make resource-usage`, tests/test_check_host.py).
#include "launch_check.h"

namespace msm_amd {

__global__ void __launch_bounds__(64) point_reset_kernel(PointCounters* __restrict__ counters) {
  uint32_t* w = reinterpret_cast<uint32_t*>(counters);
  if (threadIdx.x < 16) w[threadIdx.x] = (threadIdx.x == 6 || threadIdx.x == 7) ? 0xFFFFFFFFu : 0u;
}

__global__ void __launch_bounds__(256)
check_g1_kernel(const uint8_t* __restrict__ in, int layout, uint32_t stride, uint32_t n, uint8_t* __restrict__ reasons,
                PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) reason = check_record_g1(layout, in + (size_t)t * stride, identity);
  point_report<4>(active, t, reason, identity, reasons, counters);
}

__global__ void __launch_bounds__(64)
check_g2_kernel(const uint8_t* __restrict__ in, int ark, uint32_t n, uint32_t checks, uint8_t* __restrict__ reasons,
                PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) reason = check_record_g2(ark, in + (size_t)t * (ark ? 136 : 128), checks, identity);
  point_report<4>(active, t, reason, identity, reasons, counters);
}

void launch_point_reset(hipStream_t st, PointCounters* counters) {
  hipLaunchKernelGGL(point_reset_kernel, dim3(1), dim3(64), 0, st, counters);
}

void launch_check_g1(hipStream_t st, const void* in, int layout, uint32_t stride, uint32_t n, uint8_t* reasons,
                     PointCounters* counters) {
  hipLaunchKernelGGL(check_g1_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, (const uint8_t*)in, layout, stride, n,
                     reasons, counters);
}

void launch_check_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t checks, uint8_t* reasons,
                     PointCounters* counters) {
  hipLaunchKernelGGL(check_g2_kernel, dim3((uint32_t)(((uint64_t)n + 63) / 64)), dim3(64), 0, st, (const uint8_t*)in, ark, n, checks, reasons,
                     counters);
}

}  // namespace msm_amd
