// Launch wrappers of the point-transform kernels (k_nttp.hip) for the host driver (msm_host.hip), and the chunk
// arithmetic the driver uses to size its buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ntt_points.hip.h"

namespace msm_amd {

// work[bitrev(j)] = in[j], j < n = 2^log_n; in: records of layout_in (a host layout or PREPARED), work: packed affine
void launch_nttp_load(hipStream_t st, int layout_in, const void* in, uint32_t log_n, void* work);
// lanes [lane0, lane0 + m) of level `level`: src (packed, n records) -> 2 m XYZZ records (uppers, then lowers).  lane0 and
// m are multiples of the level's normalisation group.
void launch_nttp_level(hipStream_t st, const void* src, const void* tw, uint32_t log_n, uint32_t level, int direction,
                       uint32_t lane0, uint32_t m, void* xyzz);
// the 2 m XYZZ records of that chunk (overwritten) -> affine records of layout_out at their positions in `out`
void launch_nttp_normalise(hipStream_t st, void* xyzz, uint32_t log_n, uint32_t level, uint32_t lane0, uint32_t m,
                           int layout_out, void* out);
// xyzz[j] = [k] src[first + j] (laddered) or src[first + j] itself, j < m; k an integer
void launch_nttp_scale(hipStream_t st, const void* src, uint32_t first, uint32_t m, bool laddered, const u256& k, void* xyzz);

// host_nttp.hip: the layouts of a call (device: the _device form, which also takes PREPARED records)
bool nttp_layouts_known(bool device, int layout_in, int layout_out);

// lanes per chunk of a level for a call whose mul chunk is `mul_chunk` outputs (a multiple of kMulNormGroup): a multiple
// of kMulNormGroup, so of every level's group, or all n/2 lanes
inline uint32_t nttp_chunk_lanes(uint32_t log_n, size_t mul_chunk) {
  const size_t lanes = log_n ? (size_t)1 << (log_n - 1) : 0;
  const size_t want = std::max<size_t>(kMulNormGroup, mul_chunk / 2 / kMulNormGroup * kMulNormGroup);
  return (uint32_t)std::min(lanes, want);
}

}  // namespace msm_amd
