// Launch wrappers of the point validation kernels (k_check.hip) for the host driver (msm_host.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "check_points.hip.h"

namespace msm_amd {

// the counters of any point call (check, decompress, compress): zeroed, first_key all ones
void launch_point_reset(hipStream_t st, PointCounters* counters);
// counters: reset (launch_point_reset); reasons: n bytes or nullptr
// G1: n records of a host layout (MSM_AMD_POINT_H2C_AFFINE .. JAC_BE32), `stride` bytes each
void launch_check_g1(hipStream_t st, const void* in, int layout, uint32_t stride, uint32_t n, uint8_t* reasons,
                     PointCounters* counters);
// G2: n records, 128 B or (ark != 0) 136 B; checks: kCheckCurve, | kCheckSubgroup
void launch_check_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t checks, uint8_t* reasons,
                     PointCounters* counters);

}  // namespace msm_amd
