// The point-generic stages of the pipeline, written once for G1 and G2: the combine pass for split buckets and the
// window reduction (group sums, bit-subset sums, the host level planner).  See device_common.hip.h for the pipeline
// overview and k_reduce.hip for the reduction scheme.
//
// A stage body is templated on a traits struct G of the group:
//   G::Point, G::Ext                 internal point (PtI / PtI2) and external result (Jacobian / Jacobian2)
//   G::identity(), G::add(a, b)      the identity and the full addition
//   G::load(p), G::store(p, a)       16-byte vector accesses of a Point in global memory or LDS
//   G::to_ext(a), G::store_ext(p, e) conversion to, and store of, the external form
//   G::kReduceBitsThreads            most threads of one bit-subset sum (a power of two; LDS = threads * sizeof(Point))
// The __global__ entry points stay thin per-group wrappers beside their launch functions (k_accumulate.hip,
// k_reduce.hip: G1Stages below; k_g2.hip: its own traits), the way accumulate_kernel wraps accumulate_item.
#pragma once
#include <algorithm>

#include "device_common.hip.h"
#include "launch.h"

namespace msm_amd {

struct G1Stages {
  using Point = PtI;
  using Ext = Jacobian;
  static constexpr uint32_t kReduceBitsThreads = 512;
  static __device__ __forceinline__ Point identity() { return pti_identity(); }
  static __device__ __forceinline__ Point add(const Point& a, const Point& b) { return pti_add(a, b); }
  static __device__ __forceinline__ Point load(const Point* p) { return load_pti(p); }
  static __device__ __forceinline__ void store(Point* p, const Point& a) { store_pti(p, a); }
  static __device__ __forceinline__ Ext to_ext(const Point& a) { return pti_to_ext(a); }
  static __device__ __forceinline__ void store_ext(Ext* p, const Ext& e) { store_jac(p, e); }
};

// ---- split buckets ----------------------------------------------------------------------------------------------
// Buckets that were split into several items (only skewed digit distributions produce them: equal scalars,
// the narrow top window of small window sizes).  Two passes over multi_list:
//   combine_small  one lane per listed bucket; sums up to kSerialItems partials serially, defers
//                  larger buckets to big_list
//   combine_big    one 64-lane workgroup per deferred bucket (grid-stride): strided partial sums +
//                  6-level LDS tree
constexpr uint32_t kSerialItems = 8;

template <class G>
__device__ __forceinline__ void
combine_small_body(const uint32_t* __restrict__ multi_list, PlanCounters* __restrict__ counters,
                   const uint32_t* __restrict__ bucket_size, const uint32_t* __restrict__ item_start,
                   const uint32_t* __restrict__ win_base, uint32_t lb, uint32_t CH,
                   const typename G::Point* __restrict__ partials, typename G::Point* __restrict__ buckets,
                   uint32_t* __restrict__ big_list) {
  using P = typename G::Point;
  // the grid covers every possible split bucket (one lane each, launch_combine_pair): no grid-stride loop, fewer live
  // registers (G1: 164 VGPRs)
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= counters->multi_count) return;
  const uint32_t b = multi_list[m];
  const uint32_t nitems = (bucket_size[b] + CH - 1) / CH;
  if (nitems > kSerialItems) {
    big_list[atomicAdd(&counters->pad[0], 1u)] = b;   // pad[0] = number of deferred buckets
    return;
  }
  const P* src = partials + (size_t)win_base[b >> lb] + item_start[b];
  const P* const end = src + nitems;
  P acc = G::load(src);
#pragma unroll 1
  for (++src; src != end; ++src) acc = G::add(acc, G::load(src));
  G::store(&buckets[multi_list[m]], acc);   // b is re-read: one live register less across the loop
}

// sh: 64 Points of LDS
template <class G>
__device__ __forceinline__ void
combine_big_body(typename G::Point* sh, const uint32_t* __restrict__ big_list,
                 const PlanCounters* __restrict__ counters, const uint32_t* __restrict__ bucket_size,
                 const uint32_t* __restrict__ item_start, const uint32_t* __restrict__ win_base, uint32_t lb,
                 uint32_t CH, const typename G::Point* __restrict__ partials,
                 typename G::Point* __restrict__ buckets) {
  using P = typename G::Point;
  const uint32_t count = counters->pad[0];
  for (uint32_t m = blockIdx.x; m < count; m += gridDim.x) {
    const uint32_t b = big_list[m];
    const uint32_t nitems = (bucket_size[b] + CH - 1) / CH;
    const P* src = partials + (size_t)win_base[b >> lb] + item_start[b];
    P acc = G::identity();
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < nitems; i += 64) acc = G::add(acc, G::load(&src[i]));
    G::store(&sh[threadIdx.x], acc);
    __syncthreads();
#pragma unroll 1
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
      if (threadIdx.x < stride) {
        const P x = G::load(&sh[threadIdx.x]);
        const P y = G::load(&sh[threadIdx.x + stride]);
        G::store(&sh[threadIdx.x], G::add(x, y));
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) G::store(&buckets[b], G::load(&sh[0]));
    __syncthreads();
  }
}

// Sums the partial results of split buckets (no-op launches when nothing was split).
template <class P, class SmallKernel, class BigKernel>
void launch_combine_pair(hipStream_t st, const Plan& p, const SortBuffers& b, P* buckets, P* partials,
                         SmallKernel small_kernel, BigKernel big_kernel) {
  // multi_list doubles as big_list storage: its second half (entries max_items/2 ..) is free because a split
  // bucket accounts for at least two items
  uint32_t* big_list = b.multi_list + p.max_items / 2 + 1;
  // one lane per possibly-split bucket: at most one split bucket per two items
  hipLaunchKernelGGL(small_kernel, dim3((unsigned)((p.max_items / 2 + 63) / 64)), dim3(64), 0, st,
                     (const uint32_t*)b.multi_list, b.counters, (const uint32_t*)b.bucket_size,
                     (const uint32_t*)b.item_start, (const uint32_t*)b.win_items, p.lb, p.CH, (const P*)partials,
                     buckets, big_list);
  hipLaunchKernelGGL(big_kernel, dim3(512), dim3(64), 0, st, (const uint32_t*)big_list,
                     (const PlanCounters*)b.counters, (const uint32_t*)b.bucket_size, (const uint32_t*)b.item_start,
                     (const uint32_t*)b.win_items, p.lb, p.CH, (const P*)partials, buckets);
}

// ---- window reduction -------------------------------------------------------------------------------------------
// One job of a group-sum launch:  dst[row][q] = sum_{j < group, q*group + j < len} src[row_base(row) + (q*group + j) * elem_stride]
//   row_base(row) = (row / rows_per_window) * window_stride + (row % rows_per_window) * row_stride
// valid (level 1 only; same indexing as src): 0 = the slot was never written (the bucket matrix is not cleared per
// MSM) and counts as the identity.
template <class P>
struct GroupJob {
  const P* src;
  const uint32_t* valid;
  P* dst;
  size_t window_stride;
  uint32_t total_rows, rows_per_window, row_stride, elem_stride, len, group, out_len;
  uint32_t outputs;   // total_rows * out_len
};

// The row-sum job and the column-sum job of one level in ONE launch (they are independent; a launch costs more
// queueing behind the resident accumulate grid than the additions themselves).  One lane per output; both operands
// of every addition die in it (G1: 184 VGPRs, two waves per SIMD: it takes the place of an accumulate wave, it does
// not fit beside two).
template <class G>
__device__ __forceinline__ void sum_groups_body(const GroupJob<typename G::Point>& j0,
                                                const GroupJob<typename G::Point>& j1) {
  using P = typename G::Point;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool second = t >= j0.outputs;
  const GroupJob<P>& J = second ? j1 : j0;
  if (second) t -= j0.outputs;
  if (t >= J.outputs) return;
  const uint32_t row = t / J.out_len, q = t - row * J.out_len;
  const size_t base = (size_t)(row / J.rows_per_window) * J.window_stride + (size_t)(row % J.rows_per_window) * J.row_stride;
  const uint32_t first = q * J.group;
  const uint32_t cnt = min(J.group, J.len - first);
  P acc = G::identity();
#pragma unroll 1
  for (uint32_t j = 0; j < cnt; ++j) {
    const size_t at = base + (size_t)(first + j) * J.elem_stride;
    if (J.valid == nullptr || J.valid[at] != 0) acc = G::add(acc, G::load(&J.src[at]));
  }
  G::store(&J.dst[t], acc);
}

// grid = (lb + 1, W), one workgroup (a power of two of threads, 64..G::kReduceBitsThreads) per sum:
//   k < L      : sum of the column sums C[w][i] with bit k of i set
//   L <= k < lb: sum of the row sums R[w][i] with bit k - L of i set
//   k == lb    : sum of all row sums = the window total
// written in the external Jacobian form to out[w * (lb + 1) + k].  sh: blockDim.x Points of (dynamic) LDS.
template <class G>
__device__ __forceinline__ void
reduce_bits_body(typename G::Point* sh, const typename G::Point* __restrict__ C,
                 const typename G::Point* __restrict__ R, uint32_t L, uint32_t H, typename G::Ext* __restrict__ out) {
  using P = typename G::Point;
  const uint32_t k = blockIdx.x, w = blockIdx.y, lb = L + H;
  const bool cols = k < L;
  const uint32_t len = cols ? (1u << L) : (1u << H);
  const P* Vw = (cols ? C : R) + (size_t)w * len;
  P acc = G::identity();
  if (k == lb) {
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) acc = G::add(acc, G::load(&Vw[i]));
  } else {
    const uint32_t bit = cols ? k : k - L;
    const uint32_t half = len >> 1;
    const uint32_t lowmask = (1u << bit) - 1u;
#pragma unroll 1
    for (uint32_t j = threadIdx.x; j < half; j += blockDim.x) {
      const uint32_t i = ((j & ~lowmask) << 1) | (1u << bit) | (j & lowmask);
      acc = G::add(acc, G::load(&Vw[i]));
    }
  }
  G::store(&sh[threadIdx.x], acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t stride = blockDim.x >> 1; stride >= 1; stride >>= 1) {
    if (threadIdx.x < stride) {
      const P a = G::load(&sh[threadIdx.x]);
      const P b2 = G::load(&sh[threadIdx.x + stride]);
      G::store(&sh[threadIdx.x], G::add(a, b2));
    }
    __syncthreads();
  }
  // the host Horner pass works on the external 32-bit-limb form
  if (threadIdx.x == 0) G::store_ext(&out[(size_t)w * (lb + 1) + k], G::to_ext(G::load(&sh[0])));
}

// Threads of one bit-subset sum, at most `cap` (the group's kReduceBitsThreads).  A lone call wants the shortest
// dependency chain (one summand per thread, then the LDS tree; the loop strides where the sum is longer than the cap).
// A pipelined instance (Plan::rb_threads = 64) wants ONE wave per sum: a workgroup of two or more 182-VGPR waves needs
// that many free wave slots on one CU at once while the accumulate grid of the next instance owns the machine -- with
// one wave the reduce span of an instance drops from 1.39 to 0.88 ms at the same throughput
// (profiles/r04_reduce_bits_one_wave.txt).
inline uint32_t reduce_bits_threads(const Plan& p, uint32_t cap) {
  if (p.rb_threads) return std::min(p.rb_threads, cap);
  const uint32_t longest = 1u << ((p.lb + 1) / 2);
  uint32_t t = 64;
  while (t < cap && t < longest / 2) t <<= 1;
  return t;
}

// The levels of the window reduction:
// partial[w][0 .. L-1]      bit sums of the column sums (weights 2^k)
// partial[w][L .. L+H-1]    bit sums of the row sums    (weights 2^(L + k))
// partial[w][lb]            sum of all buckets of the window (weight 1)
template <class G, class SumGroupsKernel, class ReduceBitsKernel>
void launch_reduce_levels(hipStream_t st, const Plan& p, const typename G::Point* buckets, const uint32_t* bucket_size,
                          typename G::Point* S, typename G::Point* T, typename G::Ext* partial,
                          SumGroupsKernel sum_groups, ReduceBitsKernel reduce_bits) {
  using P = typename G::Point;
  const uint32_t L = p.red_L, H = p.red_H;
  const uint32_t ncols = 1u << L, nrows = 1u << H;
  const uint32_t min_group = std::min(std::max(p.red_group, kReduceGroupMin), kReduceGroup);
  // family 0: row sums R[w][hi] (scratch S), family 1: column sums C[w][lo] (scratch T)
  GroupJob<P> job[2];
  P* next_dst[2] = {S, T};
  for (int fam = 0; fam < 2; ++fam) {
    GroupJob<P>& J = job[fam];
    J.src = buckets;
    J.valid = bucket_size;
    J.window_stride = p.nb;
    J.rows_per_window = fam ? ncols : nrows;
    J.total_rows = p.W * J.rows_per_window;
    J.row_stride = fam ? 1u : ncols;
    J.elem_stride = fam ? ncols : 1u;
    J.len = fam ? nrows : ncols;
  }
  while (job[0].len > 1 || job[1].len > 1) {
    // per level: the smallest group (shortest chains) whose outputs still fit the lanes one launch can have resident;
    // red_group = kReduceGroup (pipelined instances) pins 16
    uint32_t group = min_group;
    while (group < kReduceGroup) {
      size_t outs = 0;
      for (int fam = 0; fam < 2; ++fam)
        if (job[fam].len > 1) outs += (size_t)job[fam].total_rows * ((job[fam].len + group - 1) / group);
      if (outs <= kReduceResidentLanes) break;
      group <<= 1;
    }
    for (int fam = 0; fam < 2; ++fam) {
      GroupJob<P>& J = job[fam];
      if (J.len > 1) {
        J.group = std::min(J.len, group);
        J.out_len = (J.len + J.group - 1) / J.group;
        J.outputs = J.total_rows * J.out_len;
        J.dst = next_dst[fam];
      } else {
        J.outputs = 0;   // this family is done
      }
    }
    const size_t outputs = (size_t)job[0].outputs + job[1].outputs;
    hipLaunchKernelGGL(sum_groups, dim3((unsigned)((outputs + 63) / 64)), dim3(64), 0, st, job[0], job[1]);
    for (int fam = 0; fam < 2; ++fam) {   // the next level reads what this one wrote: contiguous [W * rows][out_len]
      GroupJob<P>& J = job[fam];
      if (J.outputs == 0) continue;
      J.src = J.dst;
      J.valid = nullptr;
      J.window_stride = (size_t)J.rows_per_window * J.out_len;
      J.row_stride = J.out_len;
      J.elem_stride = 1;
      J.len = J.out_len;
      next_dst[fam] = J.dst + J.outputs;
    }
  }
  // job[fam].src now points at [W][rows] sums
  const uint32_t threads = reduce_bits_threads(p, G::kReduceBitsThreads);
  hipLaunchKernelGGL(reduce_bits, dim3(p.lb + 1, p.W), dim3(threads), threads * sizeof(P), st, job[1].src, job[0].src,
                     L, H, partial);
}

}  // namespace msm_amd
