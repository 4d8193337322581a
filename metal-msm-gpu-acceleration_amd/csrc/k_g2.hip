// BN254 G2 MSM kernels: the point-valued stages of the pipeline of device_common.hip.h on G2 (bn254_ec2_29.hip.h).
// The scalar front end (digits, sort, work-item planning) is the G1 one unchanged: G2 shares the scalar field Fr, so
// the work items of accumulate_g2_kernel are exactly those of accumulate_kernel.
//   convert_bases_g2_kernel   external G2 affine (128 B halo2curves / 136 B ark) -> Aff2Packed (128 B)
//   accumulate_g2_kernel      one lane per work item: mixed additions into buckets [W][nb] or item partials
//   combine_small/big_g2      the partials of split buckets
//   sum_groups_g2_kernel      row / column sums of the slot matrix (k_reduce.hip's scheme)
//   reduce_bits_g2_kernel     bit-subset sums + window totals -> partial [W][lb + 1], external Jacobian (192 B)
// A G2 point is twice the registers of a G1 point (PtI2: 72 limbs), so these kernels run at fewer waves per SIMD
// than their G1 counterparts; none of them spills (`make resource-usage`, tests/test_g2_host.py).
#include "device_common.hip.h"
#include "launch_g2.h"
#include "test_ops_g2.hip.h"

namespace msm_amd {

// 16-byte vector loads / stores of G2 records (every record size is a multiple of 16 bytes)
template <class T>
__device__ __forceinline__ T load16(const T* p) {
  static_assert(sizeof(T) % 16 == 0, "16-byte multiple");
  T r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) d[i] = q[i];
  return r;
}
template <class T>
__device__ __forceinline__ void store16(T* p, const T& a) {
  static_assert(sizeof(T) % 16 == 0, "16-byte multiple");
  uint4* q = reinterpret_cast<uint4*>(p);
  const uint4* s = reinterpret_cast<const uint4*>(&a);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) q[i] = s[i];
}

// ---- bases ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
convert_bases_g2_kernel(const uint8_t* __restrict__ in, int ark, uint32_t n, Aff2Packed* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  // 136-byte ark records are only 8-byte aligned: word loads
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in + (size_t)t * (ark ? 136 : 128));
  auto word8 = [&](int off) {
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = src[off + i];
    return r;
  };
  Affine2 a;
  a.x.c0 = word8(0);
  a.x.c1 = word8(8);
  a.y.c0 = word8(16);
  a.y.c1 = word8(24);
  if (ark && (src[32] & 0xFFu)) {   // the infinity flag (byte 128), the rule of ark_affine_to_affine_kernel
    a.x.c0 = a.x.c1 = a.y.c0 = a.y.c1 = u256_zero();
  }
  const Aff2Packed r = aff2_pack(aff2i_from_ext(a));
  store_u256(&out[t].x0, r.x0);
  store_u256(&out[t].x1, r.x1);
  store_u256(&out[t].y0, r.y0);
  store_u256(&out[t].y1, r.y1);
}

void launch_convert_bases_g2(hipStream_t st, const void* in, int ark, uint32_t n, Aff2Packed* out) {
  hipLaunchKernelGGL(convert_bases_g2_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const uint8_t*)in, ark, n, out);
}

// Precomputed window tables (build_tables_kernel of k_misc.hip on G2): tables[w * n + i] = 2^(c w) P_i as Aff2Packed,
// so that window w of scalar i adds into the SAME bucket set as window 0.  One lane per point walks the windows
// (g2_table_walk): c doublings from the previous entry, one inversion per entry.  A set-up cost, paid once per key.
__global__ void __launch_bounds__(64)
build_tables_g2_kernel(const uint8_t* __restrict__ in, int ark, uint32_t n, uint32_t c, uint32_t W,
                       Aff2Packed* __restrict__ tables) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in + (size_t)t * (ark ? 136 : 128));
  auto word8 = [&](int off) {   // word loads, as convert_bases_g2_kernel
    u256 r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = src[off + i];
    return r;
  };
  Affine2 a;
  a.x.c0 = word8(0);
  a.x.c1 = word8(8);
  a.y.c0 = word8(16);
  a.y.c1 = word8(24);
  if (ark && (src[32] & 0xFFu)) a.x.c0 = a.x.c1 = a.y.c0 = a.y.c1 = u256_zero();
  g2_table_walk(a, c, W, [&](uint32_t w, const Aff2Packed& rec) { store16(&tables[(size_t)w * n + t], rec); });
}

void launch_build_tables_g2(hipStream_t st, const void* in, int ark, uint32_t n, uint32_t c, uint32_t W,
                            Aff2Packed* tables) {
  hipLaunchKernelGGL(build_tables_g2_kernel, dim3((n + 63) / 64), dim3(64), 0, st, (const uint8_t*)in, ark, n, c, W,
                     tables);
}

// ---- accumulation -----------------------------------------------------------------------------------------------
// One lane per work item (bucket b, chunk j): points [j CH, min(size, (j + 1) CH)) of the bucket's slice of `sorted`,
// in the order `order` gives (descending length).  The state machine of accumulate_kernel: kEmpty (identity), kOne
// (one affine base: the next addition is affine + affine), kMany (a general XYZZ point: mixed additions).
__device__ __forceinline__ Aff2I g2_signed_base(const Aff2Packed* __restrict__ bases, uint32_t entry, bool& ident) {
  const Aff2Packed rec = load16(&bases[entry & 0x7FFFFFFFu]);
  ident = aff2packed_is_identity(rec);
  Aff2I q = aff2_unpack_finite(rec);
  if (entry >> 31) {   // negative digit: -y (canonical y < p -> 4 p - y < 4 p)
    q.y.c0 = Fq29::neg(q.y.c0);
    q.y.c1 = Fq29::neg(q.y.c1);
  }
  return q;
}

__global__ void __launch_bounds__(64)
accumulate_g2_kernel(const Aff2Packed* __restrict__ bases, const uint32_t* __restrict__ sorted,
                     const uint32_t* __restrict__ bucket_start, const uint32_t* __restrict__ bucket_size,
                     const uint32_t* __restrict__ item_start, const uint32_t* __restrict__ win_base,
                     const uint2* __restrict__ order, const PlanCounters* __restrict__ counters, uint32_t n,
                     uint32_t lb, uint32_t CH, PtI2* __restrict__ buckets, PtI2* __restrict__ partials) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= counters->total_items) return;
  const uint2 it = order[slot];
  const uint32_t b = it.x, j = it.y;
  const uint32_t w = b >> lb;
  const uint32_t size = bucket_size[b];
  const uint32_t lo = j * CH;
  const uint32_t cnt = min(size - lo, CH);
  const uint32_t* idx = sorted + (size_t)w * n + bucket_start[b] + lo;
  enum : uint32_t { kEmpty = 0, kOne = 1, kMany = 2 };
  uint32_t state = kEmpty;
  PtI2 acc = pt2_identity();
#pragma unroll 1
  for (uint32_t i = 0; i < cnt; ++i) {
    const uint32_t entry = idx[i];
    bool ident;
    const Aff2I q = g2_signed_base(bases, entry, ident);
    if (ident) continue;
    auto reload = [&]() {
      bool id2;
      return g2_signed_base(bases, entry, id2);
    };
    bool vanished = false;
    if (state == kMany) {
      acc = pt2_madd(acc, q.x, q.y, reload, vanished);
      if (vanished) state = kEmpty;
    } else if (state == kOne) {
      acc = pt2_mmadd(acc.x, acc.y, q.x, q.y, reload, vanished);
      state = vanished ? (uint32_t)kEmpty : (uint32_t)kMany;
    } else {
      acc = pt2_from_aff(q);
      state = kOne;
    }
  }
  if (state == kEmpty) acc = pt2_identity();
  if (size <= CH) {
    store16(&buckets[b], acc);
  } else {
    store16(&partials[(size_t)win_base[w] + item_start[b] + j], acc);
  }
}

void launch_accumulate_g2(hipStream_t st, const Plan& p, const Aff2Packed* bases, const SortBuffers& b, PtI2* buckets,
                          PtI2* partials) {
  hipLaunchKernelGGL(accumulate_g2_kernel, dim3((unsigned)((p.max_items + 63) / 64)), dim3(64), 0, st, bases,
                     (const uint32_t*)b.sorted, (const uint32_t*)b.bucket_start, (const uint32_t*)b.bucket_size,
                     (const uint32_t*)b.item_start, (const uint32_t*)b.win_items, (const uint2*)b.order,
                     (const PlanCounters*)b.counters, p.n, p.lb, p.CH, buckets, partials);
}

// ---- split buckets ----------------------------------------------------------------------------------------------
// combine_small_kernel / combine_big_kernel on G2 (k_accumulate.hip): buckets of up to kSerialItemsG2 items are summed
// serially by one lane, larger ones by one 64-lane workgroup each (strided sums + LDS tree).
constexpr uint32_t kSerialItemsG2 = 8;

__global__ void __launch_bounds__(64)
combine_small_g2_kernel(const uint32_t* __restrict__ multi_list, PlanCounters* __restrict__ counters,
                        const uint32_t* __restrict__ bucket_size, const uint32_t* __restrict__ item_start,
                        const uint32_t* __restrict__ win_base, uint32_t lb, uint32_t CH,
                        const PtI2* __restrict__ partials, PtI2* __restrict__ buckets, uint32_t* __restrict__ big_list) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= counters->multi_count) return;
  const uint32_t b = multi_list[m];
  const uint32_t nitems = (bucket_size[b] + CH - 1) / CH;
  if (nitems > kSerialItemsG2) {
    big_list[atomicAdd(&counters->pad[0], 1u)] = b;   // pad[0] = number of deferred buckets
    return;
  }
  const PtI2* src = partials + (size_t)win_base[b >> lb] + item_start[b];
  PtI2 acc = load16(src);
#pragma unroll 1
  for (uint32_t i = 1; i < nitems; ++i) acc = pt2_add(acc, load16(&src[i]));
  store16(&buckets[b], acc);
}

__global__ void __launch_bounds__(64)
combine_big_g2_kernel(const uint32_t* __restrict__ big_list, const PlanCounters* __restrict__ counters,
                      const uint32_t* __restrict__ bucket_size, const uint32_t* __restrict__ item_start,
                      const uint32_t* __restrict__ win_base, uint32_t lb, uint32_t CH,
                      const PtI2* __restrict__ partials, PtI2* __restrict__ buckets) {
  __shared__ __align__(16) PtI2 sh[64];
  const uint32_t count = counters->pad[0];
  for (uint32_t m = blockIdx.x; m < count; m += gridDim.x) {
    const uint32_t b = big_list[m];
    const uint32_t nitems = (bucket_size[b] + CH - 1) / CH;
    const PtI2* src = partials + (size_t)win_base[b >> lb] + item_start[b];
    PtI2 acc = pt2_identity();
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < nitems; i += 64) acc = pt2_add(acc, load16(&src[i]));
    store16(&sh[threadIdx.x], acc);
    __syncthreads();
#pragma unroll 1
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
      if (threadIdx.x < stride) store16(&sh[threadIdx.x], pt2_add(load16(&sh[threadIdx.x]), load16(&sh[threadIdx.x + stride])));
      __syncthreads();
    }
    if (threadIdx.x == 0) store16(&buckets[b], load16(&sh[0]));
    __syncthreads();
  }
}

void launch_combine_g2(hipStream_t st, const Plan& p, const SortBuffers& b, PtI2* buckets, PtI2* partials) {
  // big_list in the second half of multi_list, as launch_combine does (a split bucket accounts for >= 2 items)
  uint32_t* big_list = b.multi_list + p.max_items / 2 + 1;
  hipLaunchKernelGGL(combine_small_g2_kernel, dim3((unsigned)((p.max_items / 2 + 63) / 64)), dim3(64), 0, st,
                     (const uint32_t*)b.multi_list, b.counters, (const uint32_t*)b.bucket_size,
                     (const uint32_t*)b.item_start, (const uint32_t*)b.win_items, p.lb, p.CH, (const PtI2*)partials,
                     buckets, big_list);
  hipLaunchKernelGGL(combine_big_g2_kernel, dim3(512), dim3(64), 0, st, (const uint32_t*)big_list,
                     (const PlanCounters*)b.counters, (const uint32_t*)b.bucket_size, (const uint32_t*)b.item_start,
                     (const uint32_t*)b.win_items, p.lb, p.CH, (const PtI2*)partials, buckets);
}

// ---- window reduction (k_reduce.hip's scheme; see there) --------------------------------------------------------
struct GroupJobG2 {
  const PtI2* src;
  const uint32_t* valid;   // level 1: bucket_size (0 = never written = identity), later levels: nullptr
  PtI2* dst;
  size_t window_stride;
  uint32_t total_rows, rows_per_window, row_stride, elem_stride, len, group, out_len;
  uint32_t outputs;
};

__global__ void __launch_bounds__(64)
sum_groups_g2_kernel(GroupJobG2 j0, GroupJobG2 j1) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool second = t >= j0.outputs;
  const GroupJobG2& J = second ? j1 : j0;
  if (second) t -= j0.outputs;
  if (t >= J.outputs) return;
  const uint32_t row = t / J.out_len, q = t - row * J.out_len;
  const size_t base = (size_t)(row / J.rows_per_window) * J.window_stride + (size_t)(row % J.rows_per_window) * J.row_stride;
  const uint32_t first = q * J.group;
  const uint32_t cnt = min(J.group, J.len - first);
  PtI2 acc = pt2_identity();
#pragma unroll 1
  for (uint32_t j = 0; j < cnt; ++j) {
    const size_t at = base + (size_t)(first + j) * J.elem_stride;
    if (J.valid == nullptr || J.valid[at] != 0) acc = pt2_add(acc, load16(&J.src[at]));
  }
  store16(&J.dst[t], acc);
}

// grid = (lb + 1, W), blockDim.x threads (a power of two, 64..kReduceBitsG2Threads) per bit-subset sum
constexpr uint32_t kReduceBitsG2Threads = 128;   // 128 x 288 B = 36 KiB of LDS
__global__ void __launch_bounds__(kReduceBitsG2Threads)
reduce_bits_g2_kernel(const PtI2* __restrict__ C, const PtI2* __restrict__ R, uint32_t L, uint32_t H,
                      Jacobian2* __restrict__ out) {
  __shared__ __align__(16) PtI2 sh[kReduceBitsG2Threads];
  const uint32_t k = blockIdx.x, w = blockIdx.y, lb = L + H;
  const bool cols = k < L;
  const uint32_t len = cols ? (1u << L) : (1u << H);
  const PtI2* Vw = (cols ? C : R) + (size_t)w * len;
  PtI2 acc = pt2_identity();
  if (k == lb) {
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) acc = pt2_add(acc, load16(&Vw[i]));
  } else {
    const uint32_t bit = cols ? k : k - L;
    const uint32_t half = len >> 1;
    const uint32_t lowmask = (1u << bit) - 1u;
#pragma unroll 1
    for (uint32_t j = threadIdx.x; j < half; j += blockDim.x) {
      const uint32_t i = ((j & ~lowmask) << 1) | (1u << bit) | (j & lowmask);
      acc = pt2_add(acc, load16(&Vw[i]));
    }
  }
  store16(&sh[threadIdx.x], acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t stride = blockDim.x >> 1; stride >= 1; stride >>= 1) {
    if (threadIdx.x < stride) store16(&sh[threadIdx.x], pt2_add(load16(&sh[threadIdx.x]), load16(&sh[threadIdx.x + stride])));
    __syncthreads();
  }
  if (threadIdx.x == 0) store16(&out[(size_t)w * (lb + 1) + k], pt2_to_ext(load16(&sh[0])));
}

void launch_reduce_g2(hipStream_t st, const Plan& p, const PtI2* buckets, const uint32_t* bucket_size, PtI2* S, PtI2* T,
                      Jacobian2* partial) {
  const uint32_t L = p.red_L, H = p.red_H;
  const uint32_t ncols = 1u << L, nrows = 1u << H;
  const uint32_t min_group = std::min(std::max(p.red_group, kReduceGroupMin), kReduceGroup);
  GroupJobG2 job[2];
  PtI2* next_dst[2] = {S, T};
  for (int fam = 0; fam < 2; ++fam) {   // family 0: row sums (scratch S), family 1: column sums (scratch T)
    GroupJobG2& J = job[fam];
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
    uint32_t group = min_group;
    while (group < kReduceGroup) {
      size_t outs = 0;
      for (int fam = 0; fam < 2; ++fam)
        if (job[fam].len > 1) outs += (size_t)job[fam].total_rows * ((job[fam].len + group - 1) / group);
      if (outs <= kReduceResidentLanes) break;
      group <<= 1;
    }
    for (int fam = 0; fam < 2; ++fam) {
      GroupJobG2& J = job[fam];
      if (J.len > 1) {
        J.group = std::min(J.len, group);
        J.out_len = (J.len + J.group - 1) / J.group;
        J.outputs = J.total_rows * J.out_len;
        J.dst = next_dst[fam];
      } else {
        J.outputs = 0;
      }
    }
    const size_t outputs = (size_t)job[0].outputs + job[1].outputs;
    hipLaunchKernelGGL(sum_groups_g2_kernel, dim3((unsigned)((outputs + 63) / 64)), dim3(64), 0, st, job[0], job[1]);
    for (int fam = 0; fam < 2; ++fam) {
      GroupJobG2& J = job[fam];
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
  // one summand per thread where the sum is short, up to kReduceBitsG2Threads (the loop strides beyond)
  const uint32_t longest = 1u << ((p.lb + 1) / 2);
  uint32_t threads = 64;
  while (threads < kReduceBitsG2Threads && threads < longest / 2) threads <<= 1;
  hipLaunchKernelGGL(reduce_bits_g2_kernel, dim3(p.lb + 1, p.W), dim3(threads), 0, st, (const PtI2*)job[1].src,
                     (const PtI2*)job[0].src, L, H, partial);
}

// ---- raw-limb test ops (test_ops_g2.hip.h) ----------------------------------------------------------------------
__global__ void __launch_bounds__(64)
test_op_g2_kernel(int op, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                  uint32_t count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  run_test_op_g2(op, a + (size_t)t * kG2RawIn, b + (size_t)t * kG2RawIn, out + (size_t)t * kG2RawOut);
}

void launch_test_op_g2(hipStream_t st, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t count) {
  hipLaunchKernelGGL(test_op_g2_kernel, dim3((count + 63) / 64), dim3(64), 0, st, op, a, b, out, count);
}

}  // namespace msm_amd
