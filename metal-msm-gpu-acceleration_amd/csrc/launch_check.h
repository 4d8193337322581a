// Launch wrappers of the point validation kernels (k_check.hip) for the host driver (msm_host.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "check_points.hip.h"

struct msm_amd_check_report;

namespace msm_amd {

// counters: zeroed, first_key all ones (launch_check_reset); reasons: n bytes or nullptr
void launch_check_reset(hipStream_t st, CheckCounters* counters);
// G1: n records of a host layout (MSM_AMD_POINT_H2C_AFFINE .. JAC_BE32), `stride` bytes each
void launch_check_g1(hipStream_t st, const void* in, int layout, uint32_t stride, uint32_t n, uint8_t* reasons,
                     CheckCounters* counters);
// G2: n records, 128 B or (ark != 0) 136 B; checks: kCheckCurve, | kCheckSubgroup
void launch_check_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t checks, uint8_t* reasons,
                     CheckCounters* counters);

// host_check.hip: record size of a layout the checks take (G1: the four host layouts, G2: the two), 0 otherwise; and
// the report of a finished check from its counters
size_t check_stride(bool g2, int layout);
void check_report_from_counters(const CheckCounters& c, size_t n, float device_ms, msm_amd_check_report* r);

}  // namespace msm_amd
