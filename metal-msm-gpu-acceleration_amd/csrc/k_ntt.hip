// Transform kernels over BN254 Fr (ntt.hip.h):
//   ntt_twiddle_kernel  one lane per table entry: omega^j by square-and-multiply over the bits of j
//   ntt_pass_kernel     one workgroup per 2^T elements of the batch: gather, t butterfly levels, write back.  The first
//                       pass of a call converts the caller's layout and applies g^i, the last one applies n^-1 g^-i,
//                       converts back and stores to natural order.
// A thread owns four elements per step and runs two levels on them in registers (one level when t is odd and one is
// left); between steps the tile lives in LDS as eight word planes of 2^T words, so that a 32-byte record per lane is
// eight dword accesses at unit stride.  A step at slot bit b reads slots m0 + k 2^b, k < 4, m0 = the thread's group
// number with two zero bits inserted at b: within the 32 lanes of one LDS access the low five address bits then miss
// two bits (4-way conflict for b <= 3, 2-way for b = 4).  lds_pos folds slot bits 5 and 6 -- where the lanes' missing
// bits went -- back into the low five: every access of every step, and the unit-stride accesses of the gather and the
// write-back, is conflict-free.
// No scratch, no dynamically indexed register array (`make resource-usage`); the loop over steps is not unrolled.
#include "launch_ntt.h"

namespace msm_amd {

namespace {

struct NttArgs {
  const uint32_t* src;
  uint32_t* dst;
  const u256* tw;
  const u256* pow_tab;   // null: no shift
  uint64_t total;        // n_vec * n
  uint32_t log_n, level0, levels, tile_log;
  int layout;
  int first, last, direction;
  NttScale sc;
};

constexpr uint32_t kPlane = 1u << kNttTileLog;

__device__ __forceinline__ uint32_t lds_pos(uint32_t m) {
  const uint32_t u = (m >> 5) & 3u;
  return m ^ (((u * 21u) & 31u) ^ ((u >> 1) << 4));
}
__device__ __forceinline__ u256 lds_get(const uint32_t* lds, uint32_t m) {
  const uint32_t p = lds_pos(m);
  u256 x;
  MSM_UNROLL for (int w = 0; w < 8; ++w) x.v[w] = lds[w * kPlane + p];
  return x;
}
__device__ __forceinline__ void lds_put(uint32_t* lds, uint32_t m, const u256& x) {
  const uint32_t p = lds_pos(m);
  MSM_UNROLL for (int w = 0; w < 8; ++w) lds[w * kPlane + p] = x.v[w];
}

// 32-byte records of 16-byte aligned buffers move as two dwordx4
__device__ __forceinline__ u256 load_rec(const void* rec) {
  const uint4 a = ((const uint4*)rec)[0], b = ((const uint4*)rec)[1];
  u256 x;
  x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w, x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
  return x;
}
__device__ __forceinline__ void store_rec(void* rec, const u256& x) {
  ((uint4*)rec)[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  ((uint4*)rec)[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// slot bit -> bit of the flat element index (the inverse reading of ntt_slot_index)
__device__ __forceinline__ uint32_t slot_bit(const NttPass& p, uint32_t b) {
  return (b >= p.low && b < p.low + p.levels) ? p.sigma + b - p.low : b;
}

__global__ void __launch_bounds__(kNttThreads) ntt_twiddle_kernel(u256 omega, uint32_t count, u256* tw) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  u256 r = Fr::one();
  NTT_NO_UNROLL for (int b = 27; b >= 0; --b) {
    r = Fr::sqr(r);
    if ((j >> b) & 1u) r = Fr::mul(r, omega);
  }
  store_rec(tw + j, r);
}

__global__ void __launch_bounds__(kNttThreads) ntt_pass_kernel(NttArgs a) {
  __shared__ uint32_t lds[8 * kPlane];
  const NttPass p = ntt_pass(a.log_n, a.level0, a.levels, a.tile_log);
  const uint32_t slots = 1u << a.tile_log, tid = threadIdx.x;
  const uint32_t nmask = (uint32_t)(((uint64_t)1 << a.log_n) - 1u);
  const uint64_t wg = blockIdx.x;
  const bool shift = a.pow_tab != nullptr;
  // the element bits that slot bits 8 and 9 stand for: a thread's slots are tid + 256 r
  const uint32_t gb8 = slot_bit(p, 8), gb9 = slot_bit(p, 9);

  // ---- gather ----
  {
    u256 g_even = Fr::one();
    NTT_NO_UNROLL for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t m = tid + kNttThreads * r;
      if (m >= slots) break;
      const uint64_t idx = ntt_slot_index(p, wg, m);
      u256 x = u256_zero();
      if (idx < a.total) {
        x = load_rec(a.src + idx * 8);
        if (a.first) {
          x = ntt_load(a.layout, x.v);
          if (shift && a.direction == kNttForward) {   // a[i] g^i
            u256 gp;
            if (r == 0) gp = g_even = ntt_pow(a.pow_tab, (uint32_t)idx & nmask);
            else if (r == 2) gp = g_even = gb9 < a.log_n ? Fr::mul(g_even, ntt_pow2(a.pow_tab, gb9)) : g_even;
            else gp = gb8 < a.log_n ? Fr::mul(g_even, ntt_pow2(a.pow_tab, gb8)) : g_even;
            x = Fr::mul(x, gp);
          }
        }
      }
      lds_put(lds, m, x);
    }
  }
  __syncthreads();

  // ---- butterflies: steps of two levels (one at the end of an odd t) ----
  NTT_NO_UNROLL for (uint32_t lv = 0; lv < a.levels; lv += 2) {
    const bool two = lv + 1 < a.levels;
    const uint32_t level = a.level0 + lv;
    const uint32_t pb = p.low + a.levels - 1u - lv - (two ? 1u : 0u);   // lower slot bit of the step
    if (tid < (slots >> 2)) {
      uint32_t m[4];
      if (two) {
        const uint32_t m0 = ((tid >> pb) << (pb + 2)) | (tid & ((1u << pb) - 1u));
        MSM_UNROLL for (uint32_t k = 0; k < 4; ++k) m[k] = m0 + (k << pb);
      } else {   // two independent pairs
        MSM_UNROLL for (uint32_t j = 0; j < 2; ++j) {
          const uint32_t pr = 2u * tid + j;
          m[2 * j] = ((pr >> pb) << (pb + 1)) | (pr & ((1u << pb) - 1u));
          m[2 * j + 1] = m[2 * j] + (1u << pb);
        }
      }
      u256 x0 = lds_get(lds, m[0]), x1 = lds_get(lds, m[1]), x2 = lds_get(lds, m[2]), x3 = lds_get(lds, m[3]);
      const uint32_t i0 = (uint32_t)ntt_slot_index(p, wg, m[0]) & nmask;
      uint32_t tb0, tb1;
      if (two) {
        const uint32_t i1 = (uint32_t)ntt_slot_index(p, wg, m[1]) & nmask;
        const u256 ta0 = load_rec(a.tw + ntt_twiddle_index(i0, a.log_n, level));
        const u256 ta1 = load_rec(a.tw + ntt_twiddle_index(i1, a.log_n, level));
        ntt_bfly(x0, x2, ta0);
        ntt_bfly(x1, x3, ta1);
        tb0 = tb1 = ntt_twiddle_index(i0, a.log_n, level + 1u);   // elements 0 and 2 differ above the level's block
      } else {
        const uint32_t i2 = (uint32_t)ntt_slot_index(p, wg, m[2]) & nmask;
        tb0 = ntt_twiddle_index(i0, a.log_n, level);
        tb1 = ntt_twiddle_index(i2, a.log_n, level);
      }
      const u256 t0 = load_rec(a.tw + tb0);
      ntt_bfly(x0, x1, t0);
      const u256 t1 = load_rec(a.tw + tb1);
      ntt_bfly(x2, x3, t1);
      lds_put(lds, m[0], x0);
      lds_put(lds, m[1], x1);
      lds_put(lds, m[2], x2);
      lds_put(lds, m[3], x3);
    }
    __syncthreads();
  }

  // ---- write back ----
  {
    const bool inverse = a.direction == kNttInverse;
    u256 g_even = Fr::one();
    NTT_NO_UNROLL for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t m = tid + kNttThreads * r;
      if (m >= slots) break;
      const uint64_t idx = ntt_slot_index(p, wg, m);
      if (idx >= a.total) break;   // the flat index grows with the slot
      u256 x = lds_get(lds, m);
      if (!a.last) {
        store_rec(a.dst + idx * 8, x);
        continue;
      }
      const uint32_t i = (uint32_t)idx & nmask;
      const uint32_t k = a.log_n ? __brev(i) >> (32u - a.log_n) : 0u;   // position i holds X[k]
      if (inverse) {
        u256 f = a.sc.c1;   // n^-1
        if (shift) {        // (n^-1 g^-n) g^k for k != 0: element bit b is bit log_n - 1 - b of k
          if (r == 0) g_even = Fr::mul(a.sc.c0, ntt_pow(a.pow_tab, k));
          else if (r == 2 && gb9 < a.log_n) g_even = Fr::mul(g_even, ntt_pow2(a.pow_tab, a.log_n - 1u - gb9));
          u256 gp = g_even;
          if ((r & 1u) && gb8 < a.log_n) gp = Fr::mul(g_even, ntt_pow2(a.pow_tab, a.log_n - 1u - gb8));
          if (k != 0) f = gp;
        }
        x = Fr::mul(x, f);
      }
      const uint32_t j = inverse ? ((nmask + 1u - k) & nmask) : k;
      uint32_t rec[8];
      ntt_store(a.layout, x, rec);
      u256 y;
      MSM_UNROLL for (int w = 0; w < 8; ++w) y.v[w] = rec[w];
      store_rec(a.dst + ((idx - i) + j) * 8, y);
    }
  }
}

}  // namespace

void launch_ntt_twiddles(hipStream_t st, const u256& omega, uint32_t log_n, void* d_tw) {
  if (log_n == 0) return;
  const uint32_t count = 1u << (log_n - 1);
  hipLaunchKernelGGL(ntt_twiddle_kernel, dim3((count + kNttThreads - 1) / kNttThreads), dim3(kNttThreads), 0, st, omega,
                     count, (u256*)d_tw);
}

uint32_t launch_ntt(hipStream_t st, const NttLaunch& c, uint32_t max_passes) {
  const NttPlan plan = ntt_plan(c.log_n, c.tile_log);
  NttArgs a{};
  a.tw = (const u256*)c.tw;
  a.pow_tab = (const u256*)c.pow_tab;
  a.total = (uint64_t)c.n_vec << c.log_n;
  a.log_n = c.log_n, a.tile_log = c.tile_log;
  a.layout = c.layout, a.direction = c.direction;
  a.sc = c.sc;
  const uint32_t wgs = (uint32_t)((a.total + ((uint64_t)1 << c.tile_log) - 1) >> c.tile_log);
  const uint32_t run = plan.passes < max_passes ? plan.passes : max_passes;
  uint32_t level = 0;
  for (uint32_t k = 0; k < run; ++k) {
    a.first = k == 0, a.last = k + 1 == plan.passes;
    a.level0 = level, a.levels = plan.levels[k];
    // one pass: in -> out.  More: in -> scratch, scratch in place, scratch -> out (each of the earlier passes writes the
    // positions it read; only the last one permutes)
    a.src = (const uint32_t*)(a.first ? c.in : c.scratch);
    a.dst = (uint32_t*)(a.last ? c.out : c.scratch);
    hipLaunchKernelGGL(ntt_pass_kernel, dim3(wgs), dim3(kNttThreads), 0, st, a);
    level += plan.levels[k];
  }
  return run;
}

}  // namespace msm_amd
