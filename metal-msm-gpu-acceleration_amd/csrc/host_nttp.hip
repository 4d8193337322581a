// Host twin of the transform over G1 points (no ctx, no GPU): the bodies of ntt_points.hip.h on the CPU, one level of
// the network at a time, each level's butterflies split over the host threads in whole normalisation groups; the
// argument checks the twin shares with the host driver (msm_host.hip); and the twin stopped after some levels.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_ntt.h"
#include "launch_nttp.h"

namespace msm_amd {

bool nttp_layouts_known(bool device, int layout_in, int layout_out) {
  const uint32_t prepared = device ? (uint32_t)kKindPrepared : 0u;
  return point_record_bytes(false, layout_in, kKindHost | prepared) != 0 &&
         point_record_bytes(false, layout_out, kKindAffine | prepared) != 0;
}

namespace {

// One level from src (packed) into dst: records of `layout` (kLayoutPrepared for a work array) at their positions
void host_level(unsigned T, const AffPacked* src, const u256* tw, const NttpLevel& v, int direction, int layout, uint8_t* dst) {
  const uint32_t rec = point_record_bytes(false, layout, kKindAffine | kKindPrepared);
  const size_t groups = ((size_t)1 << (v.log_n - 1)) / v.group;
  for_ranges((unsigned)std::min<size_t>(T, groups), groups, [&](unsigned, size_t lo, size_t hi) {
    alignas(16) PtI recs[2 * kMulNormGroup];   // the chunk of one group of lanes: uppers, then lowers
    for (size_t g = lo; g < hi; ++g) {
      const uint32_t lane0 = (uint32_t)(g * v.group);
      for (uint32_t j = 0; j < v.group; ++j) nttp_butterfly(src, tw, v, direction, lane0 + j, recs + j, recs + v.group + j);
      for (uint32_t part = 0; part < 2; ++part) {
        uint32_t pos, stride;
        nttp_group(v, lane0, v.group, part, pos, stride);
        mul_normalise<MulG1>(recs + part * v.group, v.group, layout, stride * rec, dst + (size_t)pos * rec);
      }
    }
  });
}

// levels == kNttpAllLevels: the transform.  levels <= log_n (msm_amd_test_host_ntt_points_levels): the work array after
// that many levels, affine records of layout_out in network order, no scaling.
int host_ntt_points(int root, uint32_t log_n, int direction, int layout_in, const void* in_v, int layout_out, void* out_v,
                    int threads, uint32_t levels) {
  if (!ntt_root_known(root) || !ntt_direction_known(direction) || log_n > kNttMaxLog ||
      !nttp_layouts_known(false, layout_in, layout_out) || (levels != kNttpAllLevels && levels > log_n))
    return MSM_AMD_INPUT_ERROR;
  if (!in_v || !out_v) return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const size_t n = (size_t)1 << log_n;
  const uint32_t in_stride = point_record_bytes(false, layout_in, kKindHost),
                 out_stride = point_record_bytes(false, layout_out, kKindAffine);
  const unsigned T = worker_count(std::min(threads, 16), n);

  const u256 omega = ntt_omega(root, log_n);
  std::vector<u256> tw(n / 2);
  if (!tw.empty()) {
    u256 wtab[kNttPowEntries];
    ntt_pow_table(omega, wtab);
    for_ranges((unsigned)std::min<size_t>(T, tw.size()), tw.size(), [&](unsigned, size_t lo, size_t hi) {
      if (lo >= hi) return;
      u256 w = ntt_pow(wtab, (uint32_t)lo);
      for (size_t j = lo; j < hi; ++j) {
        tw[j] = w;
        w = Fr::mul(w, omega);
      }
    });
  }

  std::vector<AffPacked> work[2] = {std::vector<AffPacked>(n), std::vector<AffPacked>(n)};
  for_ranges(T, n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; ++j) nttp_load(layout_in, in_stride, in, log_n, (uint32_t)j, work[0].data());
  });
  const uint32_t run = levels == kNttpAllLevels ? log_n : levels;
  u256 k = u256_zero();
  const bool laddered = levels == kNttpAllLevels && direction == kNttInverse && nttp_n_inv(log_n, &k);
  const bool last_pass = laddered || run == 0;   // the records go through nttp_scale on their way out
  int cur = 0;
  for (uint32_t level = 1; level <= run; ++level) {
    const bool to_out = level == run && !last_pass;
    host_level(T, work[cur].data(), tw.data(), nttp_level(log_n, level), direction, to_out ? layout_out : kLayoutPrepared,
               to_out ? out : (uint8_t*)work[cur ^ 1].data());
    cur ^= 1;
  }
  if (!last_pass) return MSM_AMD_OK;
  const size_t groups = (n + kMulNormGroup - 1) / kMulNormGroup;
  for_ranges((unsigned)std::min<size_t>(T, groups), groups, [&](unsigned, size_t lo, size_t hi) {
    alignas(16) PtI recs[kMulNormGroup];
    for (size_t g = lo; g < hi; ++g) {
      const size_t first = g * kMulNormGroup;
      const uint32_t m = (uint32_t)std::min<size_t>(kMulNormGroup, n - first);
      for (uint32_t j = 0; j < m; ++j) recs[j] = nttp_scale(work[cur].data(), (uint32_t)(first + j), laddered, k);
      mul_normalise<MulG1>(recs, m, layout_out, out_stride, out + first * out_stride);
    }
  });
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_host_ntt_points(int root, uint32_t log_n, int direction, int point_layout_in, const void* in,
                            int point_layout_out, void* out, int threads) {
  return msm_amd::host_ntt_points(root, log_n, direction, point_layout_in, in, point_layout_out, out, threads,
                                  msm_amd::kNttpAllLevels);
}

int msm_amd_test_host_ntt_points_levels(int root, uint32_t log_n, int direction, int point_layout_in, const void* in,
                                        uint32_t levels, int point_layout_out, void* out, int threads) {
  if (levels == msm_amd::kNttpAllLevels) return MSM_AMD_INPUT_ERROR;
  return msm_amd::host_ntt_points(root, log_n, direction, point_layout_in, in, point_layout_out, out, threads, levels);
}

}  // extern "C"
