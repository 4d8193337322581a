// What the host driver (calls_points.hip) shares with the host twins of the pairing calls (host_pairing.hip).
#pragma once
#include <cstddef>
#include <cstdint>

namespace msm_amd {

bool pairing_gt_layout_known(int gt_layout);
// null, or what is wrong with the shape of a pairing product call
const char* pairing_shape_error(uint64_t n_groups, uint64_t group_size, uint32_t flags, int gt_layout, bool has_is_one);
// MSM_AMD_PAIRING_PAIRS_PER_LANE (0: not set), MSM_AMD_PAIRING_DEVICE_FINAL_FROM and MSM_AMD_PAIRING_F_IN_LDS, read at every call
void pairing_knobs(uint32_t* pairs_per_lane, uint64_t* device_final_from, bool* f_in_lds);
// n records of gt_layout -> their final exponentiations (out may be in) and, if is_one is not null, the unit flags
void host_final_exponentiation(int gt_layout, const uint8_t* in, size_t n, int threads, uint8_t* out, uint8_t* is_one);

}  // namespace msm_amd
