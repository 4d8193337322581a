// Stage 4: window reduction kernels.  See device_common.hip.h for the pipeline overview.
//
// Slot i of a window holds the bucket of digit magnitude i + 1, so the window value is  sum_i (i + 1) X[i].  With
// the slot index written as  i = hi * 2^L + lo  (L = ceil(lb / 2) column bits, H = lb - L row bits):
//     sum_i (i + 1) X[i] = sum_i X[i]  +  sum_lo lo * C[lo]  +  2^L * sum_hi hi * R[hi]
//     R[hi] = sum_lo X[hi, lo]  (row sums)        C[lo] = sum_hi X[hi, lo]  (column sums)
// Row and column sums are PLAIN sums: every bucket is added exactly twice, in independent chains of at most 7
// additions (sum_groups_kernel, groups of 16 -- per level 4..16 for a lone call --), instead of the running-sum pair "sum += X; sos += sum"
// (two dependent additions per bucket) followed by bit-subset tree sums over the segment sums (another 0.9 per
// bucket) that round 1 used: 2.0 instead of 2.9 full additions per bucket, and chains half as long.  The weights
// lo and hi are applied the same way as before: bit-subset sums over the 2^L column sums and the 2^H row sums
// (reduce_bits_kernel: tiny), whose powers of two the host Horner pass supplies with its doublings.
// Replaces sum_reduction_partial / sum_reduction_final (msm.h.metal:319-562), whose combine step needs a scalar
// multiplication per merge.
// The kernel bodies, GroupJob and the host level planner are shared with G2: point_stages.hip.h.
#include "device_common.hip.h"
#include "launch.h"
#include "point_stages.hip.h"

namespace msm_amd {

__global__ void __launch_bounds__(64)
sum_groups_kernel(GroupJob<PtI> j0, GroupJob<PtI> j1) {
  sum_groups_body<G1Stages>(j0, j1);
}

__global__ void __launch_bounds__(512)
reduce_bits_kernel(const PtI* __restrict__ C, const PtI* __restrict__ R, uint32_t L, uint32_t H,
                   Jacobian* __restrict__ out) {
  extern __shared__ uint32_t lds_u32[];
  reduce_bits_body<G1Stages>(reinterpret_cast<PtI*>(lds_u32), C, R, L, H, out);
}

// 512 threads x 144 B = 72 KiB of dynamic LDS
int reduce_set_attributes(const char** failed) {
  if (hipFuncSetAttribute((const void*)reduce_bits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024) != hipSuccess) {
    (void)hipGetLastError();
    *failed = "reduce_bits_kernel";
    return 1;
  }
  return 0;
}

// Elements of scratch one family (rows or columns) needs per window: all levels of the group sums.
size_t reduce_scratch_elems(uint32_t lb) {
  const uint32_t L = (lb + 1) / 2, H = lb - L;
  size_t need = 0;
  for (int fam = 0; fam < 2; ++fam) {
    const size_t rows = (size_t)1 << (fam ? L : H);
    uint32_t len = 1u << (fam ? H : L);
    size_t s = 0;
    while (len > 1) {   // the smallest group has the most levels and the most intermediate sums
      len = (len + kReduceGroupMin - 1) / kReduceGroupMin;
      s += rows * len;
    }
    if (s == 0) s = rows;
    need = std::max(need, s);
  }
  return need;
}

void launch_reduce(hipStream_t st, const Plan& p, const PtI* buckets, const uint32_t* bucket_size, PtI* S, PtI* T,
                   Jacobian* partial) {
  launch_reduce_levels<G1Stages>(st, p, buckets, bucket_size, S, T, partial, sum_groups_kernel, reduce_bits_kernel);
}

}  // namespace msm_amd
