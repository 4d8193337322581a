// Host twins of the scalar-multiplication kernels (no ctx, no GPU): the bodies of mul_points.hip.h on the CPU, threaded
// over ranges of whole normalisation groups, and the argument arithmetic both the twins and the host driver
// (msm_host.hip) use.
#include <hip/hip_runtime.h>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_mul.h"

namespace msm_amd {

static_assert(kMulBaseEach == MSM_AMD_MUL_BASE_EACH && kMulBaseOne == MSM_AMD_MUL_BASE_ONE, "base modes");
static_assert(MSM_AMD_SCALAR_MONT_LE == 0 && MSM_AMD_SCALAR_CANON_LE == 1 && MSM_AMD_SCALAR_CANON_BE32 == 2,
              "scalar layouts as mul_scalar reads them");
static_assert(sizeof(PtI) % 16 == 0 && sizeof(PtI2) % 16 == 0 && sizeof(AffPacked) == 64 && sizeof(Aff2Packed) == 128,
              "records move in 16-byte pieces");

bool mul_scalar_layout_known(int scalar_layout) {
  return scalar_layout >= MSM_AMD_SCALAR_MONT_LE && scalar_layout <= MSM_AMD_SCALAR_CANON_BE32;
}
size_t mul_xyzz_bytes(bool g2) { return g2 ? sizeof(PtI2) : sizeof(PtI); }
size_t mul_table_bytes(bool g2) { return (size_t)kMulTableEntries * (g2 ? sizeof(Aff2Packed) : sizeof(AffPacked)); }

namespace {

template <class G>
int host_mul(int scalar_layout, int layout_in, int base_mode, const void* scalars_v, const void* points_v, size_t n,
             int layout_out, int threads, void* out_v) {
  const size_t in_stride = point_record_bytes(G::kG2, layout_in, kKindHost), out_stride = point_record_bytes(G::kG2, layout_out, kKindAffine);
  if (!mul_scalar_layout_known(scalar_layout) || in_stride == 0 || out_stride == 0 ||
      (base_mode != kMulBaseEach && base_mode != kMulBaseOne) || n > 0xFFFFFFFFull)
    return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  if (!scalars_v || !points_v || !out_v) return MSM_AMD_INPUT_ERROR;
  const uint8_t* scalars = (const uint8_t*)scalars_v;
  const uint8_t* points = (const uint8_t*)points_v;
  uint8_t* out = (uint8_t*)out_v;
  std::vector<typename G::Packed> table;
  if (base_mode == kMulBaseOne) {
    table.resize(kMulTableEntries);
    const typename G::Aff base = G::load_base(layout_in, points);
    for_ranges(worker_count(threads, kMulTableEntries), kMulTableEntries, [&](unsigned, size_t lo, size_t hi) {
      for (size_t e = lo; e < hi; ++e) table[e] = mul_table_entry<G>(base, (uint32_t)e);
    });
  }
  const size_t groups = (n + kMulNormGroup - 1) / kMulNormGroup;
  for_ranges(worker_count(threads, groups), groups, [&](unsigned, size_t lo, size_t hi) {
    alignas(16) typename G::Pt recs[kMulNormGroup];
    for (size_t g = lo; g < hi; ++g) {
      const size_t first = g * kMulNormGroup;
      const uint32_t m = (uint32_t)std::min<size_t>(kMulNormGroup, n - first);
      for (uint32_t j = 0; j < m; ++j) {
        const size_t i = first + j;
        const u256 k = mul_scalar(scalar_layout, scalars + i * 32);
        recs[j] = base_mode == kMulBaseOne ? mul_fixed<G>(k, table.data())
                                           : mul_ladder<G>(G::load_base(layout_in, points + i * in_stride), k);
      }
      mul_normalise<G>(recs, m, layout_out, (uint32_t)out_stride, out + first * out_stride);
    }
  });
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_host_mul_points(int scalar_layout, int point_layout_in, int base_mode, const void* scalars, const void* points,
                            size_t n, int point_layout_out, int threads, void* out) {
  return msm_amd::host_mul<msm_amd::MulG1>(scalar_layout, point_layout_in, base_mode, scalars, points, n, point_layout_out,
                                           threads, out);
}

int msm_amd_host_g2_mul_points(int scalar_layout, int g2_point_layout_in, int base_mode, const void* scalars,
                               const void* points, size_t n, int g2_point_layout_out, int threads, void* out) {
  return msm_amd::host_mul<msm_amd::MulG2>(scalar_layout, g2_point_layout_in, base_mode, scalars, points, n,
                                           g2_point_layout_out, threads, out);
}

int msm_amd_test_mul_plan(int group, uint32_t out[4]) {
  if (!out || (group != 1 && group != 2)) return MSM_AMD_INPUT_ERROR;
  out[0] = msm_amd::kMulWindow;
  out[1] = msm_amd::kMulWindows;
  out[2] = msm_amd::kMulTableEntries;
  out[3] = msm_amd::kMulNormGroup;
  return MSM_AMD_OK;
}

}  // extern "C"
