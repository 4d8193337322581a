// BN254 G2 MSM kernels: the point-valued stages of the pipeline of device_common.hip.h on G2 (bn254_ec2_29.hip.h).
// The scalar front end (digits, sort, work-item planning) is the G1 one unchanged: G2 shares the scalar field Fr, so
// the work items of accumulate_g2_kernel are exactly those of accumulate_kernel.
//   convert_bases_g2_kernel   external G2 affine (128 B halo2curves / 136 B ark) -> Aff2Packed (128 B)
//   accumulate_g2_kernel      one lane per work item: mixed additions into buckets [W][nb] or item partials
//   combine_small/big_g2      the partials of split buckets                              } the bodies of
//   sum_groups_g2_kernel      row / column sums of the slot matrix                       } point_stages.hip.h,
//   reduce_bits_g2_kernel     bit-subset sums + window totals -> partial [W][lb + 1],    } instantiated with
//                             external Jacobian (192 B)                                  } G2Stages below
// The base conversion, the table build and accumulate_g2_kernel are G2's own.
// A G2 point is twice the registers of a G1 point (PtI2: 72 limbs), so these kernels run at fewer waves per SIMD
// than their G1 counterparts; none of them spills (`make resource-usage`, tests/test_g2_host.py).
#include "device_common.hip.h"
#include "launch_g2.h"
#include "point_stages.hip.h"
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

// What point_stages.hip.h needs to know about G2
struct G2Stages {
  using Point = PtI2;
  using Ext = Jacobian2;
  static constexpr uint32_t kReduceBitsThreads = 128;   // 128 x 288 B = 36 KiB of LDS: no attribute needed
  static __device__ __forceinline__ Point identity() { return pt2_identity(); }
  static __device__ __forceinline__ Point add(const Point& a, const Point& b) { return pt2_add(a, b); }
  static __device__ __forceinline__ Point load(const Point* p) { return load16(p); }
  static __device__ __forceinline__ void store(Point* p, const Point& a) { store16(p, a); }
  static __device__ __forceinline__ Ext to_ext(const Point& a) { return pt2_to_ext(a); }
  static __device__ __forceinline__ void store_ext(Ext* p, const Ext& e) { store16(p, e); }
};

// ---- bases ------------------------------------------------------------------------------------------------------
// External G2 affine record t of `in`: 128 B (halo2curves) or, ark != 0, 136 B (ark-bn254: the infinity flag at byte
// 128, the rule of ark_affine_to_affine_kernel).  136-byte records are only 8-byte aligned: word loads.
__device__ __forceinline__ Affine2 load_ext_g2(const uint8_t* __restrict__ in, int ark, uint32_t t) {
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
  if (ark && (src[32] & 0xFFu)) a.x.c0 = a.x.c1 = a.y.c0 = a.y.c1 = u256_zero();
  return a;
}

__global__ void __launch_bounds__(256)
convert_bases_g2_kernel(const uint8_t* __restrict__ in, int ark, uint32_t n, Aff2Packed* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Aff2Packed r = aff2_pack(aff2i_from_ext(load_ext_g2(in, ark, t)));
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
  const Affine2 a = load_ext_g2(in, ark, t);
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

// ---- split buckets and window reduction (point_stages.hip.h) ------------------------------------------------------
__global__ void __launch_bounds__(64)
combine_small_g2_kernel(const uint32_t* __restrict__ multi_list, PlanCounters* __restrict__ counters,
                        const uint32_t* __restrict__ bucket_size, const uint32_t* __restrict__ item_start,
                        const uint32_t* __restrict__ win_base, uint32_t lb, uint32_t CH,
                        const PtI2* __restrict__ partials, PtI2* __restrict__ buckets, uint32_t* __restrict__ big_list) {
  combine_small_body<G2Stages>(multi_list, counters, bucket_size, item_start, win_base, lb, CH, partials, buckets,
                               big_list);
}

__global__ void __launch_bounds__(64)
combine_big_g2_kernel(const uint32_t* __restrict__ big_list, const PlanCounters* __restrict__ counters,
                      const uint32_t* __restrict__ bucket_size, const uint32_t* __restrict__ item_start,
                      const uint32_t* __restrict__ win_base, uint32_t lb, uint32_t CH,
                      const PtI2* __restrict__ partials, PtI2* __restrict__ buckets) {
  __shared__ __align__(16) PtI2 sh[64];
  combine_big_body<G2Stages>(sh, big_list, counters, bucket_size, item_start, win_base, lb, CH, partials, buckets);
}

void launch_combine_g2(hipStream_t st, const Plan& p, const SortBuffers& b, PtI2* buckets, PtI2* partials) {
  launch_combine_pair(st, p, b, buckets, partials, combine_small_g2_kernel, combine_big_g2_kernel);
}

__global__ void __launch_bounds__(64)
sum_groups_g2_kernel(GroupJob<PtI2> j0, GroupJob<PtI2> j1) {
  sum_groups_body<G2Stages>(j0, j1);
}

__global__ void __launch_bounds__(G2Stages::kReduceBitsThreads)
reduce_bits_g2_kernel(const PtI2* __restrict__ C, const PtI2* __restrict__ R, uint32_t L, uint32_t H,
                      Jacobian2* __restrict__ out) {
  extern __shared__ uint4 lds_u128[];   // (16-byte aligned for load16 / store16)
  reduce_bits_body<G2Stages>(reinterpret_cast<PtI2*>(lds_u128), C, R, L, H, out);
}

void launch_reduce_g2(hipStream_t st, const Plan& p, const PtI2* buckets, const uint32_t* bucket_size, PtI2* S, PtI2* T,
                      Jacobian2* partial) {
  launch_reduce_levels<G2Stages>(st, p, buckets, bucket_size, S, T, partial, sum_groups_g2_kernel,
                                 reduce_bits_g2_kernel);
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
