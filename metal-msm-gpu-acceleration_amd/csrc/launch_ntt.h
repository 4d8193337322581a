// Launch wrappers of the transform kernels (k_ntt.hip) for the host driver (msm_host.hip), and the argument checks the
// driver shares with the host twin (host_ntt.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "ntt.hip.h"

namespace msm_amd {

// tw[j] = omega^j (Montgomery), j < n/2; nothing to do for n = 1
void launch_ntt_twiddles(hipStream_t st, const u256& omega, uint32_t log_n, void* d_tw);

struct NttLaunch {
  const void* tw;        // the domain's table
  const void* pow_tab;   // kNttPowEntries records of the shift's powers on the device, or null (no shift)
  NttScale sc;
  uint32_t log_n, tile_log;
  int direction, layout;
  const void* in;        // n_vec * n records; in == out is allowed
  void* out;
  void* scratch;         // n_vec * n records, used when the plan has more than one pass
  size_t n_vec;
};
constexpr uint32_t kNttAllPasses = ~0u;
// the first max_passes passes of one call (kNttAllPasses: the call), in stream order; returns the number of launches.
// Stopped before the last pass of its plan (msm_amd_test_ntt_passes), the state is in `scratch`: Montgomery residues
// at the positions the passes read.
uint32_t launch_ntt(hipStream_t st, const NttLaunch& c, uint32_t max_passes);

// host_ntt.hip
bool ntt_root_known(int root);
bool ntt_direction_known(int direction);
bool ntt_layout_known(int scalar_layout);   // MONT_LE and CANON_LE
// the shift record of a call (null: 1) -> reduced Montgomery residue; false: g = 0 mod r
bool ntt_read_shift(int scalar_layout, const void* shift32, u256* g);

}  // namespace msm_amd
