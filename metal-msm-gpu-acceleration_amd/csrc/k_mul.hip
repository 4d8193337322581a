// Scalar-multiplication kernels (mul_points.hip.h), one lane per record:
//   mul_table_kernel      one lane per entry of the fixed-base table: a ladder over d 2^(8 w) and one inversion
//   mul_fixed_kernel      one lane per scalar: at most 32 mixed additions from the table (L2-resident), result XYZZ
//   mul_each_kernel       one lane per (scalar, base) record: 256-step double-and-add ladder, result XYZZ
//   mul_normalise_kernel  one lane per kMulNormGroup consecutive XYZZ records: one shared inversion, affine records out
// G1 bodies run in 256-thread workgroups, G2 bodies in 64-thread ones (the register budget of the G2 kernels of this
// tree: one wave per SIMD).  None of these kernels uses scratch (`make resource-usage`, tests/test_mul_host.py).
#include "launch_mul.h"

namespace msm_amd {

template <class G>
__global__ void __launch_bounds__(64)
mul_table_kernel(int layout_in, const uint8_t* __restrict__ base, typename G::Packed* __restrict__ table) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= kMulTableEntries) return;
  G::store_packed(table + e, mul_table_entry<G>(G::load_base(layout_in, base), e));
}

template <class G>
__global__ void __launch_bounds__(G::kG2 ? 64 : 256)
mul_fixed_kernel(int scalar_layout, const uint8_t* __restrict__ scalars, uint32_t n,
                 const typename G::Packed* __restrict__ table, typename G::Pt* __restrict__ xyzz) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // n may be close to 2^32
  if (t64 >= n) return;
  const uint32_t t = (uint32_t)t64;
  G::store_pt(xyzz + t, mul_fixed<G>(mul_scalar(scalar_layout, scalars + (size_t)t * 32), table));
}

template <class G>
__global__ void __launch_bounds__(G::kG2 ? 64 : 256)
mul_each_kernel(int scalar_layout, const uint8_t* __restrict__ scalars, int layout_in, uint32_t stride,
                const uint8_t* __restrict__ points, uint32_t n, typename G::Pt* __restrict__ xyzz) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= n) return;
  const uint32_t t = (uint32_t)t64;
  const typename G::Aff a = G::load_base(layout_in, points + (size_t)t * stride);
  G::store_pt(xyzz + t, mul_ladder<G>(a, mul_scalar(scalar_layout, scalars + (size_t)t * 32)));
}

// (xyzz is read and written by the same lane: no __restrict__ pair over it)
template <class G>
__global__ void __launch_bounds__(64)
mul_normalise_kernel(typename G::Pt* xyzz, uint32_t n, int layout_out, uint32_t stride, uint8_t* out) {
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kMulNormGroup;
  if (first >= n) return;
  const uint32_t m = (uint32_t)(n - first < kMulNormGroup ? n - first : kMulNormGroup);
  mul_normalise<G>(xyzz + first, m, layout_out, stride, out + (size_t)first * stride);
}

void launch_mul_table(hipStream_t st, bool g2, int layout_in, const void* base, void* table) {
  const dim3 grid(kMulTableEntries / 64), block(64);
  if (g2)
    hipLaunchKernelGGL(mul_table_kernel<MulG2>, grid, block, 0, st, layout_in, (const uint8_t*)base, (Aff2Packed*)table);
  else
    hipLaunchKernelGGL(mul_table_kernel<MulG1>, grid, block, 0, st, layout_in, (const uint8_t*)base, (AffPacked*)table);
}

void launch_mul_fixed(hipStream_t st, bool g2, int scalar_layout, const void* scalars, uint32_t n, const void* table,
                      void* xyzz) {
  if (g2)
    hipLaunchKernelGGL(mul_fixed_kernel<MulG2>, dim3((uint32_t)(((uint64_t)n + 63) / 64)), dim3(64), 0, st, scalar_layout,
                       (const uint8_t*)scalars, n, (const Aff2Packed*)table, (PtI2*)xyzz);
  else
    hipLaunchKernelGGL(mul_fixed_kernel<MulG1>, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, scalar_layout,
                       (const uint8_t*)scalars, n, (const AffPacked*)table, (PtI*)xyzz);
}

void launch_mul_each(hipStream_t st, bool g2, int scalar_layout, const void* scalars, int layout_in, const void* points,
                     uint32_t n, void* xyzz) {
  if (g2)
    hipLaunchKernelGGL(mul_each_kernel<MulG2>, dim3((uint32_t)(((uint64_t)n + 63) / 64)), dim3(64), 0, st, scalar_layout,
                       (const uint8_t*)scalars, layout_in, point_record_bytes(true, layout_in, kKindHost | kKindPrepared), (const uint8_t*)points, n, (PtI2*)xyzz);
  else
    hipLaunchKernelGGL(mul_each_kernel<MulG1>, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, scalar_layout,
                       (const uint8_t*)scalars, layout_in, point_record_bytes(false, layout_in, kKindHost | kKindPrepared), (const uint8_t*)points, n, (PtI*)xyzz);
}

void launch_mul_normalise(hipStream_t st, bool g2, void* xyzz, uint32_t n, int layout_out, void* out) {
  const uint64_t groups = ((uint64_t)n + kMulNormGroup - 1) / kMulNormGroup;
  const dim3 grid((uint32_t)((groups + 63) / 64)), block(64);
  if (g2)
    hipLaunchKernelGGL(mul_normalise_kernel<MulG2>, grid, block, 0, st, (PtI2*)xyzz, n, layout_out,
                       point_record_bytes(true, layout_out, kKindAffine | kKindPrepared), (uint8_t*)out);
  else
    hipLaunchKernelGGL(mul_normalise_kernel<MulG1>, grid, block, 0, st, (PtI*)xyzz, n, layout_out,
                       point_record_bytes(false, layout_out, kKindAffine | kKindPrepared), (uint8_t*)out);
}

}  // namespace msm_amd
