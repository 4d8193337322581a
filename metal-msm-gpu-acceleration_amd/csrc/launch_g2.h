// Launch wrappers of the G2 kernels (k_g2.hip) and the host side of a G2 MSM (host_g2.hip), for the host driver
// (msm_host.hip).  The G2 pipeline shares the scalar front end of G1 unchanged -- scalar conversion, launch_digits,
// launch_sort and the SortBuffers they fill (launch.h) -- and replaces only the point-valued stages.
#pragma once
#include "bn254_ec2_29.hip.h"
#include "launch.h"

namespace msm_amd {

// bases: n external G2 affine records, 128 B (halo2curves G2Affine, identity = all zero) or, ark != 0, 136 B (ark-bn254
// G2Affine: x, y, then the infinity flag at byte 128) -> n Aff2Packed
void launch_convert_bases_g2(hipStream_t st, const void* in, int ark, uint32_t n, Aff2Packed* out);
// window tables of n bases in an external layout: tables[w * n + i] = 2^(c w) P_i, W * n Aff2Packed
void launch_build_tables_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t c, uint32_t W,
                            Aff2Packed* tables);
// The work items of launch_sort, one lane each, as accumulate_kernel: buckets [W][nb] or partials of split buckets
void launch_accumulate_g2(hipStream_t st, const Plan& p, const Aff2Packed* bases, const SortBuffers& b, PtI2* buckets,
                          PtI2* partials);
void launch_combine_g2(hipStream_t st, const Plan& p, const SortBuffers& b, PtI2* buckets, PtI2* partials);
// window reduction: buckets [W][nb] -> partial [W][lb + 1] (bit-subset sums, then the window total; external Jacobian);
// S, T: W * reduce_scratch_elems(lb) elements each
void launch_reduce_g2(hipStream_t st, const Plan& p, const PtI2* buckets, const uint32_t* bucket_size, PtI2* S, PtI2* T,
                      Jacobian2* partial);
void launch_test_op_g2(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count);

// host_g2.hip: Horner pass over the partial points of launch_reduce_g2 and normalisation -> 192-byte result
Jacobian2 host_combine_g2(const Jacobian2* partial, const Plan& p);

}  // namespace msm_amd
