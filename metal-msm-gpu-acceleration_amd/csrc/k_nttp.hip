// Point-transform kernels (ntt_points.hip.h):
//   nttp_load_kernel       one lane per input record: the caller's layout -> packed affine at the bit-reversed index
//   nttp_level_kernel      one lane per butterfly of a chunk of one level: a ladder (none for the factor 1) and two mixed
//                          additions, two XYZZ records out
//   nttp_normalise_kernel  one lane per normalisation group of the chunk: one shared inversion (mul_normalise), affine
//                          records out at the group's positions
//   nttp_scale_kernel      one lane per record: the uniform-scalar ladder of the INVERSE direction, XYZZ out
// 256-thread workgroups for the laddered kernels like the G1 kernels of k_mul.hip, 64 for the normalisation.  None of
// these kernels uses scratch (`make resource-usage`, tests/test_ntt_points_host.py).
#include "launch_nttp.h"

namespace msm_amd {

__global__ void __launch_bounds__(256)
nttp_load_kernel(int layout_in, uint32_t stride, const uint8_t* __restrict__ in, uint32_t log_n, AffPacked* __restrict__ work) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >> log_n) return;
  nttp_load(layout_in, stride, in, log_n, (uint32_t)j, work);
}

__global__ void __launch_bounds__(256)
nttp_level_kernel(const AffPacked* __restrict__ src, const u256* __restrict__ tw, NttpLevel v, int direction, uint32_t lane0,
                  uint32_t m, PtI* __restrict__ xyzz) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;   // m <= n/2 < 2^28
  if (t >= m) return;
  nttp_butterfly(src, tw, v, direction, lane0 + t, xyzz + t, xyzz + m + t);
}

// (xyzz is read and written by the same lane)
__global__ void __launch_bounds__(64)
nttp_normalise_kernel(PtI* xyzz, NttpLevel v, uint32_t lane0, uint32_t m, int layout_out, uint32_t rec_bytes, uint8_t* out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2u * m / v.group) return;
  uint32_t pos, stride;
  nttp_group(v, lane0, m, g, pos, stride);
  mul_normalise<MulG1>(xyzz + (size_t)g * v.group, v.group, layout_out, stride * rec_bytes, out + (size_t)pos * rec_bytes);
}

__global__ void __launch_bounds__(256)
nttp_scale_kernel(const AffPacked* __restrict__ src, uint32_t first, uint32_t m, int laddered, u256 k, PtI* __restrict__ xyzz) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  MulG1::store_pt(xyzz + t, nttp_scale(src, first + t, laddered != 0, k));
}

void launch_nttp_load(hipStream_t st, int layout_in, const void* in, uint32_t log_n, void* work) {
  const uint64_t n = (uint64_t)1 << log_n;
  hipLaunchKernelGGL(nttp_load_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, layout_in,
                     point_record_bytes(false, layout_in, kKindHost | kKindPrepared), (const uint8_t*)in, log_n, (AffPacked*)work);
}

void launch_nttp_level(hipStream_t st, const void* src, const void* tw, uint32_t log_n, uint32_t level, int direction,
                       uint32_t lane0, uint32_t m, void* xyzz) {
  hipLaunchKernelGGL(nttp_level_kernel, dim3((m + 255) / 256), dim3(256), 0, st, (const AffPacked*)src, (const u256*)tw,
                     nttp_level(log_n, level), direction, lane0, m, (PtI*)xyzz);
}

void launch_nttp_normalise(hipStream_t st, void* xyzz, uint32_t log_n, uint32_t level, uint32_t lane0, uint32_t m,
                           int layout_out, void* out) {
  const NttpLevel v = nttp_level(log_n, level);
  const uint32_t groups = 2u * m / v.group;
  hipLaunchKernelGGL(nttp_normalise_kernel, dim3((groups + 63) / 64), dim3(64), 0, st, (PtI*)xyzz, v, lane0, m, layout_out,
                     point_record_bytes(false, layout_out, kKindAffine | kKindPrepared), (uint8_t*)out);
}

void launch_nttp_scale(hipStream_t st, const void* src, uint32_t first, uint32_t m, bool laddered, const u256& k, void* xyzz) {
  hipLaunchKernelGGL(nttp_scale_kernel, dim3((m + 255) / 256), dim3(256), 0, st, (const AffPacked*)src, first, m,
                     laddered ? 1 : 0, k, (PtI*)xyzz);
}

}  // namespace msm_amd
