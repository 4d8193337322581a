// Launch wrappers of the pairing kernels (k_pairing.hip) for the host driver (calls_points.hip), and the pure planner the
// driver, the host twin (host_pairing.hip) and the tests share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace msm_amd {

constexpr uint32_t kPairingMaxPairsPerLane = 4;   // the T states one lane keeps beside its f
constexpr uint32_t kPairingFoldRadix = 4;         // lane partials one lane of a fold level multiplies
constexpr uint32_t kPairingPartialWords = 108;    // a partial product: raw limbs of an fq12 (bn254_fq12_29.hip.h)
// Group counts from which the final exponentiation runs on the device (one lane per group); below, the Miller products
// come back and the host twin finishes them.  Measured (tools/pairing_bench.py, profiles/pairing_bench.json): the device
// kernel takes 9.6 ms for any n up to 4096, sixteen host threads 3.7 ms at 256 records and 13.9 ms at 1024; the lines
// cross near 710.
constexpr uint64_t kPairingDeviceFinalFrom = 768;
// Pairs per lane: one.  At 2^14 pairs one pair per lane wins over two and four (profiles/pairing_ab.txt); sizes at which
// every SIMD already holds a lane, where sharing f's squarings could pay, have not been timed, so no default switches:
// MSM_AMD_PAIRING_PAIRS_PER_LANE asks for 2 or 4.
constexpr uint32_t kPairingDefaultPairsPerLane = 1;
// Where the running f of the Miller kernel lives by default: private memory (false) or LDS, word-major (true); the A/B at
// 2^14 pairs is in profiles/pairing_ab.txt: private memory wins, 9.64 ms of Miller + fold against 10.50.  MSM_AMD_PAIRING_F_IN_LDS = 0 / 1 asks for either.
constexpr bool kPairingFInLds = false;
constexpr uint64_t kPairingDefaultFinalFrom = ~(uint64_t)0;   // as device_final_from: stands for kPairingDeviceFinalFrom

struct PairingPlan {
  uint32_t pairs_per_lane;    // 1, 2 or 4
  uint32_t lanes_per_group;   // ceil(group_size / pairs_per_lane), at least 1 (a lane of no pairs writes the unit)
  uint32_t fold_levels;       // launches that multiply kPairingFoldRadix partials per lane until one is left
  uint32_t final_on_device;   // 1: the final exponentiation kernel runs; 0: the host twin finishes the Miller products
};

// pairs_per_lane_knob: 0 = the default, else 1, 2 or 4 (MSM_AMD_PAIRING_PAIRS_PER_LANE; anything else counts as 1);
// device_final_from: MSM_AMD_PAIRING_DEVICE_FINAL_FROM, or kPairingDefaultFinalFrom for the library's own threshold
inline PairingPlan pairing_plan(uint64_t n_groups, uint64_t group_size, uint32_t pairs_per_lane_knob,
                                uint64_t device_final_from) {
  PairingPlan p;
  if (device_final_from == kPairingDefaultFinalFrom) device_final_from = kPairingDeviceFinalFrom;
  p.pairs_per_lane = pairs_per_lane_knob == 0 ? kPairingDefaultPairsPerLane : (pairs_per_lane_knob == 2 || pairs_per_lane_knob == 4) ? pairs_per_lane_knob : 1;
  const uint64_t lanes = (group_size + p.pairs_per_lane - 1) / p.pairs_per_lane;
  p.lanes_per_group = (uint32_t)(lanes ? lanes : 1);
  p.fold_levels = 0;
  for (uint64_t c = p.lanes_per_group; c > 1; c = (c + kPairingFoldRadix - 1) / kPairingFoldRadix) ++p.fold_levels;
  p.final_on_device = n_groups >= device_final_from ? 1u : 0u;
  return p;
}

// partial[g * lanes_per_group + l] = the product of the Miller values of the pairs l ppl .. of group g (raw limbs)
void launch_pairing_miller(hipStream_t st, int layout_g1, const void* g1, int layout_g2, const void* g2, uint32_t n_groups,
                           uint32_t group_size, const PairingPlan& plan, bool f_in_lds, uint32_t* partials);
// out[g * ceil(count / radix) + j] = the product of in[g * count + radix j ..]
void launch_pairing_fold(hipStream_t st, const uint32_t* in, uint32_t n_groups, uint32_t count, uint32_t* out);
// n values -> n GT records of gt_layout (and n bytes is_one, may be null).  in_raw: raw partials, else records of
// gt_layout.  miller_only: no exponentiation, the value is only converted.
void launch_pairing_final(hipStream_t st, const void* in, bool in_raw, uint32_t n, bool miller_only, int gt_layout, void* out,
                          uint8_t* is_one);
// one lane per record of 108 words each way; count at most kTestFq12OpsMax (msm_amd_test_fq12_ops*)
constexpr uint64_t kTestFq12OpsMax = 1u << 20;
void launch_test_fq12_op(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count);

}  // namespace msm_amd
