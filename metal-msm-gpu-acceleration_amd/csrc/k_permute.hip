// Kernels of halo2's permuted lookup columns (fr_permute.hip.h); the probe that counts is that of k_lookup.hip.
//   fr_permute_reduce_kernel  one wave per tile of a level: the sum of the tile's pairs -> the tile's word of the level above.
//                             LEVEL0 reads the 32-bit counters and forms the pairs, the levels above read 64-bit words.
//   fr_permute_scan_kernel    one wave per tile: the exclusive scan of the tile, 64 words at a time (six shuffle steps and a
//                             carry), starting from the tile's word of the level above, which an earlier launch has
//                             scanned; the top level starts from 0.  Levels above 0 are scanned in place.  LEVEL0 reads
//                             the counters, writes the pairs (off, ub), stores row j at U[ub[j]] if its counter is 0, and
//                             folds rows_hit and max_multiplicity of the wave into the report.
//   fr_permute_fill_kernel    one lane per output position: fr_permute_owner, then A'[p] and S'[p] as 16-byte stores.  The
//                             lanes read the miss counter of the probe launch and store nothing if it is not zero.
//                             kPermuteHalo2 (over a sorted handle): a position that is no head takes U from its far end.
//   fr_permute_max_*_kernel   MSM_AMD_PERMUTE_FILL=scan: the heads' rows spread over their groups by a maximum scan on the
//                             same tiles, and fr_permute_fill_kernel<true> reads its owner instead of searching for it.
// Phases are ordered by launch order on one stream.  A tile walk has 2^T / 64 trips, the owner search ceil(log2 n_rows).
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

// One level of the scan.  Tile g of the launch is tile g % tiles of column g / tiles; its word of the level above is word g
// of that level, whose columns are `tiles` words long.
struct FrPermuteLevel {
  const uint32_t* counters;        // LEVEL0: n_vec columns of `len` counters
  unsigned long long* level;       // n_vec columns of `len` words: LEVEL0 the pairs (written), else this level (in place)
  unsigned long long* above;       // n_vec columns of `tiles` words; null at the top level
  uint32_t* unused;                // LEVEL0 scan: U, n_vec columns of `len` rows
  uint32_t* owner;                 // LEVEL0 scan, kPermuteFillScan: n_vec columns of owner_n cleared words; else null
  uint64_t owner_n;
  unsigned long long* report;      // LEVEL0 scan
  uint64_t len, tiles, n_tiles;    // n_tiles = n_vec tiles
  uint32_t tile_log;
};

template <bool LEVEL0>
__device__ __forceinline__ unsigned long long level_word(const FrPermuteLevel& a, uint64_t at, uint32_t* c) {
  if (!LEVEL0) return a.level[at];
  *c = a.counters[at];
  return fr_permute_pair(*c);
}

template <bool LEVEL0>
__global__ void __launch_bounds__(kPermuteThreads) fr_permute_reduce_kernel(FrPermuteLevel a) {
  const uint64_t g = ((uint64_t)blockIdx.x * kPermuteThreads + threadIdx.x) / kFrWave;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  if (g >= a.n_tiles) return;   // uniform over the wave
  const uint64_t col = g / a.tiles, first = (g - col * a.tiles) << a.tile_log;
  const uint64_t size = (uint64_t)1 << a.tile_log, left = a.len - first, have = left < size ? left : size;
  unsigned long long sum = 0;
  NTT_NO_UNROLL for (uint64_t k = lane; k < have; k += kFrWave) {
    uint32_t c;
    sum += level_word<LEVEL0>(a, col * a.len + first + k, &c);
  }
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) sum += __shfl_xor(sum, (int)d);
  if (lane == 0) a.above[g] = sum;
}

template <bool LEVEL0>
__global__ void __launch_bounds__(kPermuteThreads) fr_permute_scan_kernel(FrPermuteLevel a) {
  const uint64_t g = ((uint64_t)blockIdx.x * kPermuteThreads + threadIdx.x) / kFrWave;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  if (g >= a.n_tiles) return;   // uniform over the wave
  const uint64_t col = g / a.tiles, first = (g - col * a.tiles) << a.tile_log;
  const uint64_t size = (uint64_t)1 << a.tile_log, left = a.len - first, have = left < size ? left : size;
  unsigned long long carry = a.above ? a.above[g] : 0ull;
  uint32_t rows_hit = 0, most = 0;
  // every lane takes every trip: the shuffles need the whole wave
  NTT_NO_UNROLL for (uint64_t base = 0; base < have; base += kFrWave) {
    const uint64_t k = base + lane, at = col * a.len + first + k;
    const bool valid = k < have;
    uint32_t c = 0;
    const unsigned long long v = valid ? level_word<LEVEL0>(a, at, &c) : 0ull;
    unsigned long long incl = v;
    NTT_NO_UNROLL for (uint32_t d = 1; d < kFrWave; d <<= 1) {
      const unsigned long long other = __shfl_up(incl, d);
      if (lane >= d) incl += other;
    }
    const unsigned long long excl = carry + incl - v;
    carry += __shfl(incl, (int)kFrWave - 1);
    if (valid) a.level[at] = excl;
    if (LEVEL0) {
      // ub < len: the row's place in the list of its column's unused rows
      if (valid && c == 0) a.unused[col * a.len + fr_permute_ub(excl)] = (uint32_t)(first + k);
      // off < n while the counters of a column sum to at most n
      if (a.owner && valid && c != 0 && fr_permute_off(excl) < a.owner_n)
        a.owner[col * a.owner_n + fr_permute_off(excl)] = (uint32_t)(first + k);
      rows_hit += (uint32_t)__popcll(__ballot(valid && c != 0));
      most = c > most ? c : most;
    }
  }
  if (!LEVEL0) return;
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)most, (int)d);
    most = other > most ? other : most;
  }
  if (lane == 0 && rows_hit) {
    atomicAdd(a.report + kLookupRowsHit, (unsigned long long)rows_hit);
    atomicMax(a.report + kLookupMaxMult, (unsigned long long)most);
  }
}

// kPermuteFillScan: one level of the maximum scan over the owner words, on the same tiles.  Level 0 (the positions) is
// scanned inclusively, the levels above exclusively, all in place; 0 is the unit (row 0 owns position 0 if it owns any).
struct FrPermuteMaxLevel {
  uint32_t* level;                 // n_vec columns of `len` words
  uint32_t* above;                 // n_vec columns of `tiles` words; null at the top level
  uint64_t len, tiles, n_tiles;
  uint32_t tile_log;
  bool inclusive;
};

__global__ void __launch_bounds__(kPermuteThreads) fr_permute_max_reduce_kernel(FrPermuteMaxLevel a) {
  const uint64_t g = ((uint64_t)blockIdx.x * kPermuteThreads + threadIdx.x) / kFrWave;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  if (g >= a.n_tiles) return;   // uniform over the wave
  const uint64_t col = g / a.tiles, first = (g - col * a.tiles) << a.tile_log;
  const uint64_t size = (uint64_t)1 << a.tile_log, left = a.len - first, have = left < size ? left : size;
  uint32_t most = 0;
  NTT_NO_UNROLL for (uint64_t k = lane; k < have; k += kFrWave) {
    const uint32_t v = a.level[col * a.len + first + k];
    most = v > most ? v : most;
  }
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)most, (int)d);
    most = other > most ? other : most;
  }
  if (lane == 0) a.above[g] = most;
}

__global__ void __launch_bounds__(kPermuteThreads) fr_permute_max_scan_kernel(FrPermuteMaxLevel a) {
  const uint64_t g = ((uint64_t)blockIdx.x * kPermuteThreads + threadIdx.x) / kFrWave;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  if (g >= a.n_tiles) return;   // uniform over the wave
  const uint64_t col = g / a.tiles, first = (g - col * a.tiles) << a.tile_log;
  const uint64_t size = (uint64_t)1 << a.tile_log, left = a.len - first, have = left < size ? left : size;
  uint32_t carry = a.above ? a.above[g] : 0u;
  // every lane takes every trip: the shuffles need the whole wave
  NTT_NO_UNROLL for (uint64_t base = 0; base < have; base += kFrWave) {
    const uint64_t k = base + lane, at = col * a.len + first + k;
    const bool valid = k < have;
    uint32_t incl = valid ? a.level[at] : 0u;
    NTT_NO_UNROLL for (uint32_t d = 1; d < kFrWave; d <<= 1) {
      const uint32_t other = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d && other > incl) incl = other;
    }
    const uint32_t before = (uint32_t)__shfl_up((int)incl, 1u);
    const uint32_t mine = a.inclusive ? incl : lane ? before : 0u;
    if (valid) a.level[at] = mine > carry ? mine : carry;
    const uint32_t last = (uint32_t)__shfl((int)incl, (int)kFrWave - 1);
    carry = last > carry ? last : carry;
  }
}

struct FrPermuteFill {
  const uint32_t* rows;                  // the handle's residues
  const unsigned long long* pairs;       // n_vec columns of n_rows scanned pairs
  const uint32_t* unused;                // n_vec columns of U
  const uint32_t* counters;              // n_vec columns of n_rows counters
  const unsigned long long* report;
  uint32_t* a_out;                       // optional
  uint32_t* s_out;                       // optional
  const uint32_t* owner;                 // SCAN: n_vec columns of n scanned owner words
  uint32_t n, n_rows, total, steps;      // total = n n_vec < 2^32
  int layout;
  int arrangement;                       // kPermuteRows, kPermuteHalo2: which unused row a gap takes
};

template <bool SCAN>
__global__ void __launch_bounds__(kPermuteThreads) fr_permute_fill_kernel(FrPermuteFill a) {
  const uint64_t q = (uint64_t)blockIdx.x * kPermuteThreads + threadIdx.x;
  if (q >= a.total) return;
  // the miss counter is complete: the probe launch came before this one
  if (a.report[kLookupMissing] != 0) return;
  const uint32_t col = (uint32_t)q / a.n, p = (uint32_t)q - col * a.n;
  const unsigned long long* pairs = a.pairs + (uint64_t)col * a.n_rows;
  const uint32_t j = SCAN ? a.owner[q] : fr_permute_owner((const uint64_t*)pairs, a.n_rows, a.steps, p);
  if (SCAN && j >= a.n_rows) return;   // cannot happen: every owner word is a row index or 0
  const u256 mine = fr_store(a.layout, load_rec(a.rows + (uint64_t)j * 8));
  if (a.a_out) store_rec(a.a_out + q * 8, mine);
  if (!a.s_out) return;
  uint32_t k = 0;
  if (fr_permute_head(p, j, pairs[j], &k)) {
    store_rec(a.s_out + q * 8, mine);
    return;
  }
  // k < the number of unused rows when n == n_rows and nothing is missing; the tests hold without either being trusted
  if (k >= a.n_rows) return;
  if (a.arrangement == kPermuteHalo2) {
    const uint64_t last = (uint64_t)col * a.n_rows + a.n_rows - 1;
    const uint32_t gaps = fr_permute_unused_rows(a.pairs[last], a.counters[last]);
    if (k >= gaps) return;   // as above: cannot happen when n == n_rows and nothing is missing
    k = fr_permute_gap(a.arrangement, k, gaps);
  }
  const uint32_t r = a.unused[(uint64_t)col * a.n_rows + k];
  if (r >= a.n_rows) return;
  store_rec(a.s_out + q * 8, fr_store(a.layout, load_rec(a.rows + (uint64_t)r * 8)));
}

uint32_t wave_blocks(uint64_t waves) {
  const uint64_t per = kPermuteThreads / kFrWave;
  return (uint32_t)((waves + per - 1) / per);
}

}  // namespace

uint32_t launch_fr_lookup_permute(hipStream_t st, const FrPermuteLaunch& c) {
  uint8_t* work = (uint8_t*)c.work;
  const FrPermutePlan& p = c.plan;
  const FrScanPlan& sp = p.scan;
  uint32_t* counters = (uint32_t*)work;
  unsigned long long* report = (unsigned long long*)(work + p.report_off);
  unsigned long long* pairs = (unsigned long long*)(work + p.pairs_off);
  unsigned long long* totals = (unsigned long long*)(work + p.totals_off);
  uint32_t* unused = (uint32_t*)(work + p.u_off);
  (void)hipMemsetAsync(work, 0, p.pairs_off, st);
  (void)hipMemsetAsync(report + kLookupFirstMissing, 0xFF, 8, st);
  const bool spread = c.fill_form == kPermuteFillScan;
  const FrPermuteOwnerPlan op = fr_permute_owner_plan(p, c.n, c.n_vec, c.tile_log);
  uint32_t* owner = spread ? (uint32_t*)(work + op.owner_off) : nullptr;
  if (spread) (void)hipMemsetAsync(owner, 0, c.n * c.n_vec * 4, st);
  launch_fr_lookup_probe(st, c.probe, c.n, counters, report);
  uint32_t launches = 1;
  auto level = [&](uint32_t k) {
    FrPermuteLevel a{};
    a.counters = counters;
    a.level = k ? totals + sp.offset[k] : pairs;
    a.above = k + 1 < sp.levels ? totals + sp.offset[k + 1] : nullptr;
    a.unused = unused, a.report = report, a.owner = owner, a.owner_n = c.n;
    a.len = sp.len[k], a.tiles = sp.tiles[k], a.n_tiles = sp.tiles[k] * c.n_vec, a.tile_log = c.tile_log;
    return a;
  };
  for (uint32_t k = 0; k + 1 < sp.levels; ++k, ++launches) {
    const FrPermuteLevel a = level(k);
    if (k == 0) hipLaunchKernelGGL(fr_permute_reduce_kernel<true>, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
    else hipLaunchKernelGGL(fr_permute_reduce_kernel<false>, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
  }
  for (uint32_t k = sp.levels; k-- != 0; ++launches) {
    const FrPermuteLevel a = level(k);
    if (k == 0) hipLaunchKernelGGL(fr_permute_scan_kernel<true>, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
    else hipLaunchKernelGGL(fr_permute_scan_kernel<false>, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
  }
  if (spread) {
    uint32_t* totals32 = (uint32_t*)(work + op.totals_off);
    auto max_level = [&](uint32_t k) {
      FrPermuteMaxLevel a{};
      a.level = k ? totals32 + op.scan.offset[k] : owner;
      a.above = k + 1 < op.scan.levels ? totals32 + op.scan.offset[k + 1] : nullptr;
      a.len = op.scan.len[k], a.tiles = op.scan.tiles[k], a.n_tiles = op.scan.tiles[k] * c.n_vec, a.tile_log = c.tile_log;
      a.inclusive = k == 0;
      return a;
    };
    for (uint32_t k = 0; k + 1 < op.scan.levels; ++k, ++launches) {
      const FrPermuteMaxLevel a = max_level(k);
      hipLaunchKernelGGL(fr_permute_max_reduce_kernel, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
    }
    for (uint32_t k = op.scan.levels; k-- != 0; ++launches) {
      const FrPermuteMaxLevel a = max_level(k);
      hipLaunchKernelGGL(fr_permute_max_scan_kernel, dim3(wave_blocks(a.n_tiles)), dim3(kPermuteThreads), 0, st, a);
    }
  }
  FrPermuteFill f{};
  f.owner = owner;
  f.rows = (const uint32_t*)((const uint8_t*)c.probe.image + c.probe.plan.rows_off);
  f.pairs = pairs, f.unused = unused, f.counters = counters, f.report = report, f.arrangement = c.arrangement;
  f.a_out = (uint32_t*)c.a_out, f.s_out = (uint32_t*)c.s_out;
  f.n = (uint32_t)c.n, f.n_rows = (uint32_t)c.probe.n_rows, f.total = (uint32_t)(c.n * c.n_vec), f.steps = p.search_steps;
  f.layout = c.probe.layout;
  const dim3 grid((uint32_t)((c.n * c.n_vec + kPermuteThreads - 1) / kPermuteThreads));
  if (spread) hipLaunchKernelGGL(fr_permute_fill_kernel<true>, grid, dim3(kPermuteThreads), 0, st, f);
  else hipLaunchKernelGGL(fr_permute_fill_kernel<false>, grid, dim3(kPermuteThreads), 0, st, f);
  return launches + 1;
}

}  // namespace msm_amd
