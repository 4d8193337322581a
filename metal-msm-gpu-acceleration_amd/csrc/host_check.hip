// Host twins of the point validation kernels (no ctx, no GPU): the bodies of check_points.hip.h on the CPU, threaded
// over index ranges, and the report arithmetic both the twins and the host driver (msm_host.hip) use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/msm_amd.h"
#include "launch_check.h"

namespace msm_amd {

static_assert(kPointValid == MSM_AMD_POINT_VALID && kPointNotReduced == MSM_AMD_POINT_NOT_REDUCED &&
                  kPointNotOnCurve == MSM_AMD_POINT_NOT_ON_CURVE && kPointNotInSubgroup == MSM_AMD_POINT_NOT_IN_SUBGROUP,
              "reason codes of check_points.hip.h and msm_amd.h");
static_assert(kCheckCurve == MSM_AMD_CHECK_CURVE && kCheckSubgroup == MSM_AMD_CHECK_SUBGROUP, "check mask bits");
static_assert(kLayoutH2cAffine == MSM_AMD_POINT_H2C_AFFINE && kLayoutArkProjective == MSM_AMD_POINT_ARK_PROJECTIVE &&
                  kLayoutArkAffine == MSM_AMD_POINT_ARK_AFFINE && kLayoutJacBe32 == MSM_AMD_POINT_JAC_BE32,
              "G1 layouts of check_points.hip.h and msm_amd.h");

// record size of a layout the checks take (the four G1 host layouts / the two G2 host layouts), 0 otherwise
size_t check_stride(bool g2, int layout) {
  if (g2) return msm_amd_g2_point_bytes(layout);
  return layout >= MSM_AMD_POINT_H2C_AFFINE && layout <= MSM_AMD_POINT_JAC_BE32 ? msm_amd_point_bytes(layout) : 0;
}

void check_report_from_counters(const CheckCounters& c, size_t n, float device_ms, msm_amd_check_report* r) {
  *r = msm_amd_check_report{};
  r->n_checked = n;
  for (int k = 0; k < 4; ++k) r->by_reason[k] = c.by_reason[k];
  r->n_invalid = (uint64_t)c.by_reason[1] + c.by_reason[2] + c.by_reason[3];
  r->n_identity = c.n_identity;
  const bool none = c.first_key == ~0ull;
  r->first_invalid = none ? UINT64_MAX : (c.first_key >> 2);
  r->first_reason = none ? 0u : (uint32_t)(c.first_key & 3u);
  r->device_ms = device_ms;
}

namespace {

int host_check(bool g2, int layout, const void* points, size_t n, uint32_t checks, int threads, uint8_t* reasons,
               msm_amd_check_report* report) {
  const size_t stride = check_stride(g2, layout);
  if (!report || stride == 0 || checks == 0 || (checks & ~(uint32_t)(kCheckCurve | kCheckSubgroup)) ||
      n > 0xFFFFFFFFull || (n > 0 && !points))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)points;
  const unsigned want = threads > 0 ? (unsigned)threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(want, n));
  std::vector<CheckCounters> part(T);
  const size_t chunk = (n + T - 1) / T;
  auto worker = [&](unsigned t) {
    CheckCounters c{};
    c.first_key = ~0ull;
    const size_t lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
    for (size_t i = lo; i < hi; ++i) {
      bool identity = false;
      const uint32_t reason = g2 ? check_record_g2(layout == MSM_AMD_G2_POINT_ARK_AFFINE, in + i * stride, checks, identity)
                                 : check_record_g1(layout, in + i * stride, identity);
      if (reasons) reasons[i] = (uint8_t)reason;
      ++c.by_reason[reason];
      c.n_identity += identity;
      if (reason != kPointValid) c.first_key = std::min<uint64_t>(c.first_key, ((uint64_t)i << 2) | reason);
    }
    part[t] = c;
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker, t);
  worker(0);
  for (std::thread& th : pool) th.join();
  CheckCounters sum{};
  sum.first_key = ~0ull;
  for (const CheckCounters& c : part) {
    for (int k = 0; k < 4; ++k) sum.by_reason[k] += c.by_reason[k];
    sum.n_identity += c.n_identity;
    sum.first_key = std::min(sum.first_key, c.first_key);
  }
  check_report_from_counters(sum, n, 0.0f, report);
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
