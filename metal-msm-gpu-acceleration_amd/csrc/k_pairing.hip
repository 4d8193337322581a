// Pairing kernels (bn254_fq12_29.hip.h), one lane per unit of work, 64-thread workgroups:
//   pairing_miller_kernel  one lane per pairs_per_lane pairs of one group: the 64 steps of the optimal ate loop over the
//                          signed digits of 6x + 2, f squared once per step for all the lane's pairs, then the two
//                          Frobenius steps; the lane's partial product goes out as raw limbs
//   pairing_fold_kernel    one lane per kPairingFoldRadix partials of a group: one level of the product tree; the host
//                          launches level after level, nothing waits on another workgroup
//   pairing_final_kernel   one lane per group: the final exponentiation, the unit test, the conversion to the record
//   test_fq12_op_kernel    msm_amd_test_fq12_op
// State: the T of every pair and the operands of a product live in the lane's private memory, which the compiler
// places in scratch; the running f of the Miller loop too, or, in the other instantiation, in LDS (see the kernel); the products walk them with rolled loops, so the code stays small and the registers hold the
// 2 x 17 column sums of one Fq2 accumulation.
#include <type_traits>

#include "launch_pairing.h"
#include "bn254_fq12_29.hip.h"
#include "mul_points.hip.h"

namespace msm_amd {

struct PairState {
  g2proj T;
  g2aff Q, Qn;   // Q and -Q
  g1eval P;
};

// LDS_F: the running f sits in LDS, word-major [word][lane] (108 x 64 words = 27 KB per workgroup of one wave), and the
// squaring and the line multiplications reach it there; else it is an fq12 of the lane's private memory.
template <bool LDS_F>
__global__ void __launch_bounds__(64)
pairing_miller_kernel(int layout_g1, uint32_t stride_g1, const uint8_t* __restrict__ g1, int layout_g2, uint32_t stride_g2,
                      const uint8_t* __restrict__ g2, uint32_t n_groups, uint32_t group_size, uint32_t ppl, uint32_t lpg,
                      uint32_t* __restrict__ partials) {
  __shared__ uint32_t lds_f[LDS_F ? kPairingPartialWords * 64 : 1];
  using Store = typename std::conditional<LDS_F, Fq12Strided, Fq12Private>::type;
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= (uint64_t)n_groups * lpg) return;
  const uint32_t g = (uint32_t)(t64 / lpg), lane = (uint32_t)(t64 % lpg);
  const uint64_t first = (uint64_t)lane * ppl;
  const uint32_t want = first < group_size ? (uint32_t)(group_size - first < ppl ? group_size - first : ppl) : 0u;
  PairState s[kPairingMaxPairsPerLane];
  uint32_t live = 0;   // pairs with neither point the identity, packed to the front of s
  MSM_NO_UNROLL for (uint32_t i = 0; i < want && i < kPairingMaxPairsPerLane; ++i) {
    const uint64_t rec = (uint64_t)g * group_size + first + i;
    const AffI p = MulG1::load_base(layout_g1, g1 + rec * stride_g1);
    const Aff2I q = MulG2::load_base(layout_g2, g2 + rec * stride_g2);
    if (MulG1::aff_is_identity(p) || MulG2::aff_is_identity(q)) continue;
    PairState& e = s[live++];
    e.P = g1eval{p.x, p.y};
    e.Q = g2aff{q.x, q.y};
    e.Qn = g2aff{q.x, Fq2::sub<4>(Fq2::zero(), q.y)};
    e.T = g2proj{q.x, q.y, Fq2::one()};
  }
  fq12 f_private;
  Store f;
  if constexpr (LDS_F) {
    (void)f_private;
    f = Fq12Strided{lds_f + threadIdx.x, 64u};
  } else {
    f = Fq12Private{&f_private};
  }
  fq12_set_one_t(f);
  line_coeffs l;
  if (live) {
    MSM_NO_UNROLL for (int b = 63; b >= 0; --b) {
      if (b != 63) fq12_sqr_t(f);
      const bool pos = (kAtePos >> b) & 1u, neg = (kAteNeg >> b) & 1u;
      MSM_NO_UNROLL for (uint32_t i = 0; i < live; ++i) {
        double_step(s[i].T, l, s[i].P);
        fq12_mul_line_t(f, l);
        if (pos || neg) {
          add_step(s[i].T, l, pos ? s[i].Q : s[i].Qn, s[i].P);
          fq12_mul_line_t(f, l);
        }
      }
    }
    MSM_NO_UNROLL for (uint32_t i = 0; i < live; ++i) {
      g2aff q1, q2;
      g2_frob_points(s[i].Q, q1, q2);
      add_step(s[i].T, l, q1, s[i].P);
      fq12_mul_line_t(f, l);
      add_step(s[i].T, l, q2, s[i].P);
      fq12_mul_line_t(f, l);
    }
  }
  fq12_to_raw_t(partials + (size_t)t64 * kPairingPartialWords, f);
}

__global__ void __launch_bounds__(64)
pairing_fold_kernel(const uint32_t* __restrict__ in, uint32_t n_groups, uint32_t count, uint32_t out_count,
                    uint32_t* __restrict__ out) {
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= (uint64_t)n_groups * out_count) return;
  const uint32_t g = (uint32_t)(t64 / out_count), j = (uint32_t)(t64 % out_count);
  const uint64_t first = (uint64_t)j * kPairingFoldRadix;
  const uint32_t m = (uint32_t)(count - first < kPairingFoldRadix ? count - first : kPairingFoldRadix);
  const uint32_t* src = in + ((size_t)g * count + first) * kPairingPartialWords;
  fq12 f, x;
  fq12_from_raw(f, src);
  MSM_NO_UNROLL for (uint32_t i = 1; i < m; ++i) {
    fq12_from_raw(x, src + (size_t)i * kPairingPartialWords);
    fq12_mul(f, f, x);
  }
  fq12_to_raw(out + (size_t)t64 * kPairingPartialWords, f);
}

__global__ void __launch_bounds__(64)
pairing_final_kernel(const uint32_t* in, int in_raw, uint32_t n, int miller_only, int gt_layout,
                     uint32_t* out, uint8_t* is_one) {   // out may be in: a lane reads its record before it writes
  const uint64_t t64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t64 >= n) return;
  fq12 f;
  if (in_raw)
    fq12_from_raw(f, in + (size_t)t64 * kPairingPartialWords);
  else
    fq12_from_record(f, in + (size_t)t64 * (kGtBytes / 4), gt_layout);
  if (!miller_only) fq12_final_exp(f);
  if (is_one) is_one[t64] = fq12_is_one(f) ? 1 : 0;
  fq12_to_record(out + (size_t)t64 * (kGtBytes / 4), f, gt_layout);
}

__global__ void __launch_bounds__(64)
test_fq12_op_kernel(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                    uint32_t count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  run_test_fq12_op(op, a + (size_t)t * kFq12Words, b + (size_t)t * kFq12Words, out + (size_t)t * kFq12Words);
}

static dim3 lanes_grid(uint64_t lanes) { return dim3((uint32_t)((lanes + 63) / 64)); }

void launch_pairing_miller(hipStream_t st, int layout_g1, const void* g1, int layout_g2, const void* g2, uint32_t n_groups,
                           uint32_t group_size, const PairingPlan& plan, bool f_in_lds, uint32_t* partials) {
  hipLaunchKernelGGL(f_in_lds ? pairing_miller_kernel<true> : pairing_miller_kernel<false>, lanes_grid((uint64_t)n_groups * plan.lanes_per_group), dim3(64), 0, st, layout_g1,
                     point_record_bytes(false, layout_g1, kKindHost | kKindPrepared), (const uint8_t*)g1, layout_g2,
                     point_record_bytes(true, layout_g2, kKindHost | kKindPrepared), (const uint8_t*)g2, n_groups, group_size,
                     plan.pairs_per_lane, plan.lanes_per_group, partials);
}

void launch_pairing_fold(hipStream_t st, const uint32_t* in, uint32_t n_groups, uint32_t count, uint32_t* out) {
  const uint32_t out_count = (count + kPairingFoldRadix - 1) / kPairingFoldRadix;
  hipLaunchKernelGGL(pairing_fold_kernel, lanes_grid((uint64_t)n_groups * out_count), dim3(64), 0, st, in, n_groups, count,
                     out_count, out);
}

void launch_pairing_final(hipStream_t st, const void* in, bool in_raw, uint32_t n, bool miller_only, int gt_layout, void* out,
                          uint8_t* is_one) {
  hipLaunchKernelGGL(pairing_final_kernel, lanes_grid(n), dim3(64), 0, st, (const uint32_t*)in, in_raw ? 1 : 0, n,
                     miller_only ? 1 : 0, gt_layout, (uint32_t*)out, is_one);
}

void launch_test_fq12_op(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count) {
  hipLaunchKernelGGL(test_fq12_op_kernel, dim3((count + 63) / 64), dim3(64), 0, st, op, a, b, out, count);
}

}  // namespace msm_amd
