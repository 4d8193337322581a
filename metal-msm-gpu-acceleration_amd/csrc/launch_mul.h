// Launch wrappers of the scalar-multiplication kernels (k_mul.hip) for the host driver (msm_host.hip), and the argument
// arithmetic the driver shares with the host twins (host_mul.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "mul_points.hip.h"

namespace msm_amd {

// the fixed-base table of ONE base record (an input layout of the group): kMulTableEntries packed affine entries
void launch_mul_table(hipStream_t st, bool g2, int layout_in, const void* base, void* table);
// xyzz[i] = [s_i] P from the table of P; scalars: n records of 32 B in scalar_layout
void launch_mul_fixed(hipStream_t st, bool g2, int scalar_layout, const void* scalars, uint32_t n, const void* table, void* xyzz);
// xyzz[i] = [s_i] P_i; points: n records of an input layout of the group
void launch_mul_each(hipStream_t st, bool g2, int scalar_layout, const void* scalars, int layout_in, const void* points,
                     uint32_t n, void* xyzz);
// n XYZZ records (overwritten) -> n affine records of layout_out, one inversion per kMulNormGroup consecutive records
void launch_mul_normalise(hipStream_t st, bool g2, void* xyzz, uint32_t n, int layout_out, void* out);

// host_mul.hip
bool mul_scalar_layout_known(int scalar_layout);
size_t mul_xyzz_bytes(bool g2);
size_t mul_table_bytes(bool g2);

}  // namespace msm_amd
