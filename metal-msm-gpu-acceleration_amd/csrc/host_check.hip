// Host twins of the point validation kernels (no ctx, no GPU): the bodies of check_points.hip.h on the CPU, threaded
// over index ranges; the report is the counter fold of point_report.hip.h.
#include <hip/hip_runtime.h>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_check.h"

namespace msm_amd {

static_assert(kPointValid == MSM_AMD_POINT_VALID && kPointNotReduced == MSM_AMD_POINT_NOT_REDUCED &&
                  kPointNotOnCurve == MSM_AMD_POINT_NOT_ON_CURVE && kPointNotInSubgroup == MSM_AMD_POINT_NOT_IN_SUBGROUP &&
                  kPointBadEncoding == MSM_AMD_POINT_BAD_ENCODING,
              "reason codes of point_report.hip.h and msm_amd.h");
static_assert(kCheckCurve == MSM_AMD_CHECK_CURVE && kCheckSubgroup == MSM_AMD_CHECK_SUBGROUP, "check mask bits");
static_assert(kLayoutH2cAffine == MSM_AMD_POINT_H2C_AFFINE && kLayoutArkProjective == MSM_AMD_POINT_ARK_PROJECTIVE &&
                  kLayoutArkAffine == MSM_AMD_POINT_ARK_AFFINE && kLayoutJacBe32 == MSM_AMD_POINT_JAC_BE32 &&
                  kLayoutPrepared == MSM_AMD_POINT_PREPARED && kG2LayoutH2cAffine == MSM_AMD_G2_POINT_H2C_AFFINE &&
                  kG2LayoutArkAffine == MSM_AMD_G2_POINT_ARK_AFFINE && kG2LayoutPrepared == MSM_AMD_G2_POINT_PREPARED,
              "layouts of check_points.hip.h and msm_amd.h");

namespace {

int host_check(bool g2, int layout, const void* points, size_t n, uint32_t checks, int threads, uint8_t* reasons,
               msm_amd_check_report* report) {
  const size_t stride = point_record_bytes(g2, layout, kKindHost);
  if (!report || stride == 0 || checks == 0 || (checks & ~(uint32_t)(kCheckCurve | kCheckSubgroup)) ||
      n > 0xFFFFFFFFull || (n > 0 && !points))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)points;
  const unsigned T = worker_count(threads, n);
  std::vector<PointCounters> part(T);
  for_ranges(T, n, [&](unsigned t, size_t lo, size_t hi) {
    PointCounters c = point_counters_empty();
    for (size_t i = lo; i < hi; ++i) {
      bool identity = false;
      const uint32_t reason = g2 ? check_record_g2(layout == MSM_AMD_G2_POINT_ARK_AFFINE, in + i * stride, checks, identity)
                                 : check_record_g1(layout, in + i * stride, identity);
      if (reasons) reasons[i] = (uint8_t)reason;
      point_counters_add(c, i, reason, identity);
    }
    part[t] = c;
  });
  PointCounters sum = point_counters_empty();
  for (const PointCounters& c : part) point_counters_merge(sum, c);
  point_report_decode(sum, n, 0.0f, report);
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_host_check_points(int point_layout, const void* points, size_t n, uint32_t checks, int threads,
                              uint8_t* reasons, msm_amd_check_report* report) {
  return msm_amd::host_check(false, point_layout, points, n, checks, threads, reasons, report);
}

int msm_amd_host_g2_check_points(int g2_point_layout, const void* points, size_t n, uint32_t checks, int threads,
                                 uint8_t* reasons, msm_amd_check_report* report) {
  return msm_amd::host_check(true, g2_point_layout, points, n, checks, threads, reasons, report);
}

}  // extern "C"
