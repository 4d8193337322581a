// Kernels of the sort of Fr records by canonical value (fr_sort.hip.h):
//   fr_sort_keys_kernel      one lane per record of the call: the canonical key into ctx-owned memory, the digit mask (against
//                            the key of record 0, formed once per workgroup and shared through LDS) folded by a per-wave OR
//                            and one atomic OR per wave.
//   fr_sort_gather_kernel    one lane per position of a column: the pair (word w of key[perm[i]], perm[i]); perm is the second
//                            word of the pair that is there already, or the identity before the first pass.
//   fr_sort_hist_kernel      one workgroup per tile of 4096 pairs: the tile's count of each of the 256 digits.
//   fr_sort_row_scan_kernel  one workgroup per digit: the exclusive scan of that digit's counts over the tiles, and its total.
//   fr_sort_scatter_kernel   one workgroup per tile: each wave owns a contiguous quarter of the tile, so wave order is memory
//                            order; the lanes of a wave that hold the same digit rank themselves by eight ballots, the lowest
//                            of them moves the wave's cursor.  Stable.
//   fr_sort_final_kernel     one lane per sorted position: the record of key[perm[k]] in the caller's layout and perm[k].
// Phases are ordered by launch order on one stream; the columns of a call follow each other and share the pairs and the
// histograms.  Every index read from a pair is checked against n before it addresses memory, and so is every position a pair
// is scattered to.
#include <utility>

#include "launch_fr.h"

namespace msm_amd {

namespace {

__device__ __forceinline__ u256 load_rec(const uint32_t* rec) {
  const uint4 a = ((const uint4*)rec)[0], b = ((const uint4*)rec)[1];
  u256 x;
  x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w, x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
  return x;
}
__device__ __forceinline__ void store_rec(uint32_t* rec, const u256& x) {
  ((uint4*)rec)[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  ((uint4*)rec)[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

__global__ void __launch_bounds__(kSortThreads) fr_sort_keys_kernel(int layout, const uint32_t* in, uint64_t total,
                                                                     uint32_t* keys, uint32_t* record) {
  const uint64_t i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  // the key of record 0 (total >= 1): formed by the first lane of the workgroup, so that three of its four waves do not pay
  // a second reduction, and shared through LDS
  __shared__ uint32_t first_key[8];
  if (threadIdx.x == 0) {
    const u256 k = fr_sort_key(layout, load_rec(in));
    MSM_UNROLL for (int w = 0; w < 8; ++w) first_key[w] = k.v[w];
  }
  __syncthreads();
  u256 key0;
  MSM_UNROLL for (int w = 0; w < 8; ++w) key0.v[w] = first_key[w];
  uint32_t m = 0;
  if (i < total) {
    const u256 key = fr_sort_key(layout, load_rec(in + i * 8));
    store_rec(keys + i * 8, key);
    m = fr_sort_diff(key, key0);
  }
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) m |= (uint32_t)__shfl_xor((int)m, (int)d);
  if (lane == 0 && m) atomicOr(record, m);
}

__global__ void __launch_bounds__(kSortThreads) fr_sort_gather_kernel(const uint32_t* keys, uint2* pairs, uint32_t n, uint32_t w,
                                                                       bool first) {
  const uint64_t i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = first ? (uint32_t)i : pairs[i].y;
  // p < n: the pairs are a permutation of the identity; one that is not is kept and addresses nothing
  pairs[i] = make_uint2(p < n ? keys[(uint64_t)p * 8 + w] : 0u, p);
}

__global__ void __launch_bounds__(kSortThreads) fr_sort_hist_kernel(const uint2* in, uint32_t n, uint32_t shift, uint32_t tiles,
                                                                     uint32_t* tile_hist /* [256][tiles] */) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
  NTT_NO_UNROLL for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint64_t i = base + (uint64_t)r * kSortThreads + threadIdx.x;
    if (i < n) atomicAdd(&h[(in[i].x >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  tile_hist[(uint64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of one word per thread over a workgroup of `waves` <= 16 waves; scratch: 17 words of LDS
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
  const uint32_t lane = threadIdx.x & (kFrWave - 1), wave = threadIdx.x / kFrWave, waves = blockDim.x / kFrWave;
  uint32_t incl = v;
  NTT_NO_UNROLL for (uint32_t d = 1; d < kFrWave; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == kFrWave - 1) scratch[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    NTT_NO_UNROLL for (uint32_t k = 0; k < waves; ++k) {
      const uint32_t s = scratch[k];
      scratch[k] = run;
      run += s;
    }
    scratch[16] = run;
  }
  __syncthreads();
  const uint32_t res = scratch[wave] + incl - v;
  *total = scratch[16];
  __syncthreads();
  return res;
}

__global__ void __launch_bounds__(1024) fr_sort_row_scan_kernel(uint32_t* tile_hist, uint32_t tiles, uint32_t* digit_total) {
  __shared__ uint32_t scratch[17];
  uint32_t* row = tile_hist + (uint64_t)blockIdx.x * tiles;
  uint32_t carry = 0;
  NTT_NO_UNROLL for (uint32_t base = 0; base < tiles; base += blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < tiles ? row[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_scan(v, scratch, &total);
    if (i < tiles) row[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) digit_total[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kSortThreads) fr_sort_scatter_kernel(const uint2* in, uint2* out, uint32_t n, uint32_t shift,
                                                                        uint32_t tiles, const uint32_t* tile_offset,
                                                                        const uint32_t* digit_total) {
  __shared__ uint32_t wh[4][256];   // per-wave digit counts, then per-wave write cursors
  __shared__ uint32_t scratch[17];
  uint32_t all;
  const uint32_t digit_base = block_scan(digit_total[threadIdx.x], scratch, &all);
  const uint32_t lane = threadIdx.x & (kFrWave - 1), wave = threadIdx.x / kFrWave;
  for (int v = 0; v < 4; ++v) wh[v][threadIdx.x] = 0;
  __syncthreads();
  const uint64_t wbase = (uint64_t)blockIdx.x * kSortTile + (uint64_t)wave * (kSortTile / 4);
  NTT_NO_UNROLL for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint64_t i = wbase + (uint64_t)r * kFrWave + lane;
    if (i < n) atomicAdd(&wh[wave][(in[i].x >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  {
    // thread d turns the four per-wave counts of digit d into write positions
    uint32_t run = digit_base + tile_offset[(uint64_t)threadIdx.x * tiles + blockIdx.x];
    for (int v = 0; v < 4; ++v) {
      const uint32_t cnt = wh[v][threadIdx.x];
      wh[v][threadIdx.x] = run;
      run += cnt;
    }
  }
  __syncthreads();
  // every lane takes every trip: the ballots need the whole wave
  NTT_NO_UNROLL for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint64_t i = wbase + (uint64_t)r * kFrWave + lane;
    const bool valid = i < n;
    uint2 item = make_uint2(0, 0);
    if (valid) item = in[i];
    const uint32_t d = (item.x >> shift) & 0xFFu;
    unsigned long long same = __ballot(valid);
    MSM_UNROLL for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long bal = __ballot((d >> bit) & 1u);
      same &= ((d >> bit) & 1u) ? bal : ~bal;
    }
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint32_t rank = (uint32_t)__popcll(same & below);
    uint32_t pos = 0;
    if (valid) pos = wh[wave][d] + rank;
    // the lowest lane of each digit group moves the wave's cursor (LDS operations of one wave are ordered)
    if (valid && rank == 0) wh[wave][d] += (uint32_t)__popcll(same);
    if (valid && pos < n) out[pos] = item;   // pos < n: the counts of all tiles and digits sum to n
  }
}

__global__ void __launch_bounds__(kSortThreads) fr_sort_final_kernel(int layout, const uint32_t* keys, const uint2* pairs,
                                                                      uint32_t n, uint32_t* out, uint32_t* perm_out) {
  const uint64_t k = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x;
  if (k >= n) return;
  const uint32_t p = pairs ? pairs[k].y : (uint32_t)k;
  if (p >= n) return;   // cannot happen: the pairs are a permutation of the identity
  if (out) store_rec(out + k * 8, fr_sort_record(layout, load_rec(keys + (uint64_t)p * 8)));
  if (perm_out) perm_out[k] = p;
}

uint32_t blocks_of(uint64_t items) { return (uint32_t)((items + kSortThreads - 1) / kSortThreads); }

}  // namespace

void launch_fr_sort_keys(hipStream_t st, const FrSortLaunch& c) {
  uint8_t* work = (uint8_t*)c.work;
  const uint64_t total = c.n * c.n_vec;
  (void)hipMemsetAsync(work, 0, kSortRecordBytes, st);
  hipLaunchKernelGGL(fr_sort_keys_kernel, dim3(blocks_of(total)), dim3(kSortThreads), 0, st, c.layout, (const uint32_t*)c.in,
                     total, (uint32_t*)(work + c.plan.keys_off), (uint32_t*)work);
}

uint32_t launch_fr_sort_passes(hipStream_t st, const FrSortLaunch& c, uint32_t mask) {
  uint8_t* work = (uint8_t*)c.work;
  const uint32_t n = (uint32_t)c.n, tiles = (uint32_t)c.plan.tiles;
  uint32_t* tile_hist = (uint32_t*)(work + c.plan.hist_off);
  uint32_t* digit_total = tile_hist + (uint64_t)tiles * 256;
  uint32_t launches = 0;
  for (uint64_t v = 0; v < c.n_vec; ++v) {
    const uint32_t* keys = (const uint32_t*)(work + c.plan.keys_off) + v * c.n * 8;
    uint2* src = (uint2*)(work + c.plan.pairs_off);
    uint2* dst = src + c.n;
    bool first = true;
    for (uint32_t w = 0; w < 8; ++w) {
      const uint32_t bits = (mask >> (4 * w)) & 0xFu;
      if (!bits) continue;
      hipLaunchKernelGGL(fr_sort_gather_kernel, dim3(blocks_of(n)), dim3(kSortThreads), 0, st, keys, src, n, w, first);
      first = false, ++launches;
      for (uint32_t b = 0; b < 4; ++b) {
        if (!((bits >> b) & 1u)) continue;
        hipLaunchKernelGGL(fr_sort_hist_kernel, dim3(tiles), dim3(kSortThreads), 0, st, (const uint2*)src, n, 8 * b, tiles,
                           tile_hist);
        hipLaunchKernelGGL(fr_sort_row_scan_kernel, dim3(256), dim3(1024), 0, st, tile_hist, tiles, digit_total);
        hipLaunchKernelGGL(fr_sort_scatter_kernel, dim3(tiles), dim3(kSortThreads), 0, st, (const uint2*)src, dst, n, 8 * b, tiles,
                           (const uint32_t*)tile_hist, (const uint32_t*)digit_total);
        std::swap(src, dst);
        launches += 3;
      }
    }
    hipLaunchKernelGGL(fr_sort_final_kernel, dim3(blocks_of(n)), dim3(kSortThreads), 0, st, c.layout, keys,
                       first ? (const uint2*)nullptr : (const uint2*)src, n,
                       c.out ? (uint32_t*)c.out + v * c.n * 8 : (uint32_t*)nullptr, c.perm_out ? c.perm_out + v * c.n : nullptr);
    ++launches;
  }
  return launches;
}

}  // namespace msm_amd
