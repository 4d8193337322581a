// Compressed-point kernels (compress_points.hip.h), one lane per record, 256-thread workgroups:
//   decompress_g1_kernel   32-byte records -> affine (halo2curves / ark) or prepared 64-byte records: one Fq root
//   decompress_g2_kernel   64-byte records -> affine or prepared 128-byte records: two Fq roots and one inversion
//   compress_g1_kernel / compress_g2_kernel   affine records -> compressed records (two / four Montgomery reductions)
//   sqrt_raw_kernel        the root bodies at raw limbs (MSM_AMD_RAW_FE_SQRT, MSM_AMD_G2_RAW_FQ2_SQRT)
// Report: point_report<5> of point_report.hip.h.  An invalid record still gets an output: the layout's identity
// encoding.  None of these kernels uses scratch (`make resource-usage`, tests/test_gpu_compress.py).
#include "launch_compress.h"

namespace msm_amd {

__global__ void __launch_bounds__(256)
decompress_g1_kernel(const uint8_t* __restrict__ in, int format, uint32_t n, int layout, uint32_t stride,
                     uint8_t* __restrict__ out, uint8_t* __restrict__ reasons, PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) {
    AffI pt;
    reason = decompress_record_g1(format, in + (size_t)t * 32, pt, identity);
    decompress_store_g1(layout, out + (size_t)t * stride, pt);
  }
  point_report<5>(active, t, reason, identity, reasons, counters);
}

__global__ void __launch_bounds__(256)
decompress_g2_kernel(const uint8_t* __restrict__ in, int format, uint32_t n, int layout, uint32_t stride,
                     uint8_t* __restrict__ out, uint8_t* __restrict__ reasons, PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  uint32_t reason = kPointValid;
  bool identity = false;
  if (active) {
    Aff2I pt;
    reason = decompress_record_g2(format, in + (size_t)t * 64, pt, identity);
    decompress_store_g2(layout, out + (size_t)t * stride, pt);
  }
  point_report<5>(active, t, reason, identity, reasons, counters);
}

// records written as all 0xFF are counted in by_reason[kPointNotReduced]: one ballot and one atomic per wave
__device__ __forceinline__ void compress_count_bad(bool bad, PointCounters* __restrict__ counters) {
  const uint64_t m = __ballot(bad);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&counters->by_reason[kPointNotReduced], (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(256)
compress_g1_kernel(const uint8_t* __restrict__ in, int layout, uint32_t stride, uint32_t n, int format,
                   uint8_t* __restrict__ out, PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  bool bad = false;
  if (active) bad = compress_record_g1(layout, in + (size_t)t * stride, format, out + (size_t)t * 32);
  compress_count_bad(bad, counters);
}

__global__ void __launch_bounds__(256)
compress_g2_kernel(const uint8_t* __restrict__ in, int layout, uint32_t stride, uint32_t n, int format,
                   uint8_t* __restrict__ out, PointCounters* __restrict__ counters) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t64 < n;
  const uint32_t t = (uint32_t)t64;
  bool bad = false;
  if (active) bad = compress_record_g2(layout, in + (size_t)t * stride, format, out + (size_t)t * 64);
  compress_count_bad(bad, counters);
}

__global__ void __launch_bounds__(64)
sqrt_raw_kernel(int g2, const uint32_t* __restrict__ a, uint32_t* __restrict__ out, uint32_t count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  if (g2) raw_sqrt_fq2(a + (size_t)t * 72, out + (size_t)t * 80);
  else raw_sqrt_fq(a + (size_t)t * 36, out + (size_t)t * 40);
}

static dim3 compress_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + 255) / 256)); }

void launch_decompress(hipStream_t st, bool g2, int format, const void* in, uint32_t n, int layout, uint32_t stride,
                       void* out, uint8_t* reasons, PointCounters* counters) {
  if (g2)
    hipLaunchKernelGGL(decompress_g2_kernel, compress_grid(n), dim3(256), 0, st, (const uint8_t*)in, format, n, layout, stride,
                       (uint8_t*)out, reasons, counters);
  else
    hipLaunchKernelGGL(decompress_g1_kernel, compress_grid(n), dim3(256), 0, st, (const uint8_t*)in, format, n, layout, stride,
                       (uint8_t*)out, reasons, counters);
}

void launch_compress(hipStream_t st, bool g2, int layout, uint32_t stride, const void* in, uint32_t n, int format, void* out,
                     PointCounters* counters) {
  if (g2)
    hipLaunchKernelGGL(compress_g2_kernel, compress_grid(n), dim3(256), 0, st, (const uint8_t*)in, layout, stride, n, format,
                       (uint8_t*)out, counters);
  else
    hipLaunchKernelGGL(compress_g1_kernel, compress_grid(n), dim3(256), 0, st, (const uint8_t*)in, layout, stride, n, format,
                       (uint8_t*)out, counters);
}

void launch_sqrt_raw(hipStream_t st, bool g2, const uint32_t* a, uint32_t* out, uint32_t count) {
  hipLaunchKernelGGL(sqrt_raw_kernel, dim3((count + 63) / 64), dim3(64), 0, st, g2 ? 1 : 0, a, out, count);
}

}  // namespace msm_amd
