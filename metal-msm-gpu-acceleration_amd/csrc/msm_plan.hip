// The planner of the MSM driver: the window policies (pipelined, lone, bounded, tables), the Plan of one instance and of
// the window reduction alone, the geometry of a window table, and the exports that are nothing but planner.  Nothing here
// touches the device.  The environment switches of make_plan, instance_plan and pick_reduce_group are read per call: the
// tests set them between calls on one ctx.  What the other units of the driver call is in msm_amd::drv (msm_driver.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "msm_driver.h"

namespace {

uint32_t auto_window(size_t n) {
  // The reference uses 3 below 32 points and 15 from there on (msm.rs:137-141).  Measured on MI355X in pipelined
  // batches (ms per MSM, round 2 -- the row / column-sum reduction made buckets cheaper, which moved every
  // boundary one size down): 2^12 c=5 0.23 | 2^14 c=5 0.24 | 2^16 c=13 0.33 | 2^18 c=15 0.47 (16: 0.50) |
  // 2^19 c=16 0.79 (15: 0.80, 17: 0.84) | 2^20 c=17 1.41 (16: 1.43, 15: 1.54) | 2^21 c=17 2.72 (16: 2.83) |
  // 2^22 c=17 5.82 (16: 6.21).  Windows whose TOP digit is narrow are traps: the n entries of the top window then
  // share a handful of buckets (c = 14 leaves 2 bits for the top window of a 254-bit scalar, c = 11 one bit: 2^17
  // points cost 1.2 ms with c = 10 or 11, 0.38 with 15).
  if (n < 32) return 3;   // msm.rs:137-138
  const uint32_t l = floor_log2(n);
  if (l <= 14) return 5;
  if (l <= 18) return 15;   // 2^16 in batches of 40 after the 64-bit host pass: c=15 0.207, c=13 0.233, c=16 0.246 ms per MSM
  if (l == 19) return 16;   // u32 digits from here on
  return kMaxWindow;
}

// Window size of a LONE call (one instance, nothing else in flight: lone_call()).  The pipelined policy above minimises
// GPU work per MSM; a lone call is a chain of launches and of dependent point additions, where a wide window costs
// little (the window reduction is a fixed number of levels, the accumulate kernel is far from filling the machine)
// and a narrow top window costs a lot (split buckets -> the combine pass).  Median ms of one blocking device-resident
// call on MI355X (tools/lone_latency.py, profiles/r02_lone_call_window_sweep.txt), best | pipelined policy:
//   2^8 c=8 0.346 | c=5 0.357     2^12 c=8 0.446 | c=5 0.538     2^14 c=15 0.487 | c=5 0.596
//   2^16 c=15 0.543 | c=13 0.661  2^18 c=15 0.810 (16: 0.796)    2^19 c=17 1.201 | c=16 1.253
uint32_t auto_window_lone(size_t n) {
  if (n < 32) return 3;
  const uint32_t l = floor_log2(n);
  if (l <= 6) return 5;
  if (l <= 12) return 8;
  if (l <= 18) return 15;
  return kMaxWindow;
}

// `windows` = 0: the per-call pipeline (every signed-digit window owns a bucket set).  `windows` > 0: the
// precomputed-table pipeline of a table with that many windows, where the [W_digits][n_scalars] digit matrix is sorted
// as ONE window of W_digits * n_scalars entries whose "point index" addresses the table entry 2^(c w) P_i directly (the
// table is window-major: a bounded call's W_digits windows are a prefix of it).
// `width`: magnitudes stay below 2^width.width() (scalar_width.hip.h) -- W_digits = width / c + 1 windows, of which the
// top one holds at most c - 1 bits and so absorbs the last carry (254 bits: ceil(255 / c)).  Everything below follows
// from W_digits, W and n.
Plan make_plan(size_t n_scalars, uint32_t c, uint32_t windows = 0, WidthBound width = WidthBound{}) {
  Plan p{};
  p.c = c;
  p.W_digits = width.width() / c + 1;
  if (!(width.bits == kScalarBits && !width.sign)) p.bits = width.bits, p.sign = width.sign;   // 254 unsigned: the unbounded plan
  if (windows) windows = std::min(windows, p.W_digits);
  const size_t n = windows ? n_scalars * windows : n_scalars;
  p.n = (uint32_t)n;
  p.W = windows ? 1u : p.W_digits;
  p.n_scalars = (uint32_t)n_scalars;
  p.wide_digits = c > 15;
  p.lb = std::max(c - 1, (uint32_t)kSegLog);
  p.nb = 1u << p.lb;                  // slot i <-> digit magnitude i + 1 (c = 3 is padded to 8 slots)
  // sort / planning workgroup size: big workgroups are the fastest alone, but they can hardly be placed while
  // an accumulate grid of another instance is resident (they need 16 free wave slots on one CU at once)
  p.front_threads = 1024;
  if (const char* e = std::getenv("MSM_AMD_FRONT_THREADS")) {
    const int v = std::atoi(e);
    if (v == 256 || v == 512 || v == 1024) p.front_threads = (uint32_t)v;
  }
  // sort pass 1: one workgroup per (chunk, window); about 2 x 1024 threads per CU in total
  uint32_t Q = std::max(1u, (512u * (1024u / p.front_threads)) / p.W);
  const uint32_t max_q = (uint32_t)((n + 4095) / 4096);
  Q = std::max(1u, std::min(Q, max_q));
  p.Q = Q;
  p.chunk = (uint32_t)((((n + Q - 1) / Q) + 63) & ~(size_t)63);
  // Sort geometry.  Pass 2 sorts a region inside LDS, so the coarse passes must cut a window into regions of
  // ~16 k entries: T = ceil(log2(n / 16384)) coarse bits.  Up to 7 bits (128 regions) one coarse pass does it
  // (every per-call plan up to 2^21 points); beyond that the bits are split over TWO coarse passes of <= 6 bits
  // each (hb + mb, three-level sort): one pass with 1024 regions keeps too many partially written lines open
  // (2^24 points: 10.2 ms), and 128 regions of 131 k entries force pass 2 to scatter in global memory (6.0 ms).
  uint32_t T = 0;
  while (T + 2 < p.lb && (n >> T) > 16384) ++T;
  uint32_t hb = T, mb = 0;
  if (T > 7) {
    hb = (T + 1) / 2;
    mb = T - hb;
  }
  if (const char* e = std::getenv("MSM_AMD_HB")) {   // experiments: coarse bits of the two-pass sort
    const int v = std::atoi(e);
    if (v >= 0 && (uint32_t)v + 2 <= p.lb) {
      hb = (uint32_t)v;
      mb = 0;
    }
  }
  if (const char* e = std::getenv("MSM_AMD_MB")) {   // experiments: middle-pass bits
    const int v = std::atoi(e);
    if (v >= 0 && hb + (uint32_t)v + 2 <= p.lb) mb = (uint32_t)v;
  }
  p.hb = hb;
  p.mb = mb;
  p.fb = p.lb - hb - mb;
  if (p.fb > 10) {   // the fine histogram is scanned with one bin per thread (<= 1024 bins)
    const uint32_t extra = p.fb - 10;
    p.fb = 10;
    if (p.mb || p.hb + extra > 7) p.mb += extra; else p.hb += extra;
  }
  // what pass 1 leaves in the u16 tmp_fine is mb + fb bits
  while (p.mb + p.fb > 16) {
    ++p.hb;
    --p.mb;
  }
  // Tile-staged scatter (k_sort.hip tile_scatter): 26 % less sort time for ONE huge instance (2^24 points: 7.0 ->
  // 5.2 ms with 1024-thread workgroups), but its 60 VGPRs x 1024 threads cannot be placed beside a resident
  // accumulate grid, so inside a pipeline of instances it loses (headline 695 -> 643 MSM/s; with 512 threads: no
  // difference to the direct scatter).  Used where the sort is not hidden behind another instance's accumulation:
  // per-call plans that need the three-level sort (2^22 points and more).
  p.tiled = (p.mb != 0 && windows == 0) ? 1u : 0u;
  if (const char* e = std::getenv("MSM_AMD_TILED")) p.tiled = std::atoi(e) != 0;
  p.tile_threads = 1024;
  if (const char* e = std::getenv("MSM_AMD_TILE_THREADS")) {
    const int v = std::atoi(e);
    if (v == 256 || v == 512 || v == 1024) p.tile_threads = (uint32_t)v;
  }
  p.ballot = kDefaultBallot;
  if (const char* e = std::getenv("MSM_AMD_BALLOT")) p.ballot = (uint32_t)std::atoi(e) & 3u;
  // front-end traffic: digits_hist_kernel counts the digits it has just made, and where index, sign and fine digit
  // fit one u32 (headline: 20 + 1 + 10 bits) pass 1 hands pass 2 one array instead of two (k_sort.hip)
  p.fused_front = windows == 0;
  p.packed = p.mb == 0 && n >= 1 && floor_log2(std::max<size_t>(n - 1, 1)) + 1 + 1 + p.fb <= 32;
  p.Q2 = 1;
  if (p.mb) {
    const uint32_t regions = p.W << p.hb;
    p.Q2 = std::max(1u, 1024u / regions);
    while (p.Q2 > 1 && (n >> p.hb) / p.Q2 < 4096) p.Q2 >>= 1;
  }
  // accumulate work items: at most CH points each; buckets longer than CH are cut into several items whose partial
  // sums the combine kernels add up (one extra full addition per cut, and a second affine+affine start).  Uniform
  // scalars must split (almost) nothing: CH >= mean + 5 sigma of the Poisson bucket size (2^20 points, c = 16: mean
  // 32, CH = 64; the round-1 rule picked 32 there and cut 228 k of 524 k buckets in two).  Only when the buckets
  // alone cannot fill the chip twice (2 waves/SIMD x 1024 SIMDs x 64 lanes = 131 k lanes per round) are items made
  // shorter on purpose.  Skewed inputs (equal scalars, narrow top windows) still get cut at CH.
  const double mean_len = (double)n / (double)p.nb;
  uint32_t ch = 16;
  while (ch < 512 && (double)ch < mean_len + 5.0 * std::sqrt(mean_len)) ch <<= 1;
  while (ch > 16 && (size_t)p.W * p.nb + ((size_t)p.W * n) / ch < 262144) ch >>= 1;
  if (const char* e = std::getenv("MSM_AMD_CH")) {
    const int v = std::atoi(e);
    if (v >= 16 && v <= 512 && (v & (v - 1)) == 0) ch = (uint32_t)v;
  }
  p.CH = ch;
  p.red_L = (p.lb + 1) / 2;
  p.red_H = p.lb - p.red_L;
  p.red_group = kReduceGroup;
  p.total_buckets = (size_t)p.W * p.nb;
  p.total_segs = (size_t)p.W * reduce_scratch_elems(p.lb);   // scratch elements of each of the two sum families
  p.max_items = p.total_buckets + ((size_t)p.W * n) / ch + 1;
  p.partial_count = (size_t)p.W * (p.lb + 1);
  return p;
}

// Row / column sums of the window reduction for a LONE call: with no neighbouring instance to fill the machine, the
// 15-addition chains of the pipelined setting (one lane per 16 buckets: 35 k lanes at 2^18 points, 7.7 k in the second
// level at 2^20) are pure latency.  launch_reduce then takes, level by level, the smallest group (>= this minimum) whose
// outputs still fit the lanes one launch can have resident; a further level costs one launch (~5 us), one addition
// in a chain about 6 us.
uint32_t pick_reduce_group(const Plan&) {
  if (const char* e = std::getenv("MSM_AMD_REDUCE_GROUP")) return (uint32_t)std::atoi(e);
  return kReduceGroupMin;
}

}  // namespace
namespace msm_amd { namespace drv __attribute__((visibility("hidden"))) {
uint32_t floor_log2(size_t n) {
  uint32_t l = 0;
  while ((n >> (l + 1)) != 0) ++l;
  return l;
}

// Window of a bounded call (msm_amd_msm_bounded*).  254 bits: the two policies above.  Below: read from the sweep of every
// window 3..17 at 2^16, 2^18, 2^20, 2^22 points x 1, 8, 16, 32, 64, 128 bits, lone and pipelined, uniform scalars below
// 2^bits on prepared bases (tools/bounded_bench.py --sweep, profiles/bounded_sweep.txt; ms per MSM).  What it shows:
//  - the window count W = bits / c + 1 decides first: every window sorts and accumulates all n entries.  One window
//    that holds the whole scalar (c = bits + 1, no digit is ever negative) is the fastest form of every width up to 16:
//    8 bits c = 9 (2^22 pipelined 0.57; c = 17: 5.87, c = 5: 2.68), 16 bits c = 17 (2^22: 0.56; c = 9: 0.83, c = 15: 7.4);
//  - the trap of auto_window is much deeper here, because a short scalar has few other windows to hide it behind: a top
//    digit of t = bits - (W - 1) c bits puts n entries into 2^t buckets.  32 bits at 2^20 pipelined: c = 17 (t = 15)
//    0.35, c = 16 (the top window holds the carry alone) 2.2, c = 13 (t = 6) 1.45.  The rule below takes the fewest
//    windows among the c whose top digit is full (t = c - 1) or wide enough that a bucket stays below the longest work
//    item (2^t >= n / 512), and the widest top digit if there is none;
//  - at 2^16 and 2^18 points the 2^16 buckets per window of c = 17 cost more than a fifth window saves: 64 and 128 bits
//    want c = 13 there (2^18 lone 64 bits: 0.455 | c = 17 0.499; 128 bits: 0.674 | 0.791; pipelined 0.233 | 0.282 and
//    0.367 | 0.593), and so does every width in a pipeline of 2^16-point instances (32 bits: c = 11 0.163 | c = 17 0.204);
//  - 128 bits from 2^20 points: c = 10 (W = 13, t = 8) beats the rule's c = 13 at 2^20 (pipelined 1.22 | 1.83, lone
//    1.94 | 2.78) and ties with it at 2^22 (4.31 | 4.15, lone 5.50 | 5.77): no reading of the other cells explains it,
//    so it stands as an exception for the width of a 128-bit challenge alone;
//  - one bit: no window differs by more than the spread (every point lands in slot 1; 2^20 lone 4.49 .. 4.52).
// Cells where the rule is not the fastest window: 2^16 pipelined 16 bits (c = 9 0.179 | c = 6 0.152), 2^18 pipelined
// 16 bits (c = 17 0.199 | c = 9 0.181), 2^22 pipelined 128 bits (above); all others within 3 %.  Sizes below 2^15 were
// not swept: they keep the window of the unbounded call (and still run bits / c + 1 windows of it).
uint32_t auto_window_bounded(size_t n, uint32_t bits, bool lone) {
  const uint32_t c0 = lone ? auto_window_lone(n) : auto_window(n);
  if (bits >= kModulusBits) return c0;
  const uint32_t l = floor_log2(n);
  if (l < 15) return c0;
  uint32_t cmax = (uint32_t)kMaxWindow;
  if ((!lone && l <= 17) || (l <= 18 && bits / kMaxWindow + 1 >= 4)) cmax = 13;
  if (l >= 19 && bits > 124 && bits <= 128) return 10;
  if (bits + 1 <= cmax) return std::max<uint32_t>(kMinWindow, bits + 1);   // one window, every digit positive
  uint32_t best = cmax, best_W = 0, best_t = 0;
  bool best_ok = false;
  for (uint32_t c = 9; c <= cmax; ++c) {
    const uint32_t W = bits / c + 1, t = bits - (W - 1) * c;
    const bool ok = t >= std::min(c - 1, l > 9 ? l - 9 : 0u);
    bool take;
    if (ok != best_ok) take = ok;
    else if (ok) take = best_W == 0 || W < best_W || (W == best_W && l >= 19);   // ties: the larger window from 2^19 points
    else take = best_W == 0 || t > best_t || (t == best_t && l >= 19);
    if (take) best = c, best_W = W, best_t = t, best_ok = ok;
  }
  return best;
}

// Geometry of the window reduction alone (stage entry point sum_reduction).
Plan make_reduce_plan(uint32_t lb, uint32_t W) {
  Plan p{};
  p.c = lb + 1;   // only used to space bit positions in host_combine (one window at a time)
  p.W = W;
  p.lb = lb;
  p.nb = 1u << lb;
  p.red_L = (lb + 1) / 2;
  p.red_H = lb - p.red_L;
  p.red_group = kReduceGroup;
  p.total_buckets = (size_t)p.W * p.nb;
  p.total_segs = (size_t)p.W * reduce_scratch_elems(lb);
  p.partial_count = (size_t)p.W * (lb + 1);
  return p;
}

// window_size 0 = `auto_c`; the window and the number of windows of a table over n points
int tables_geometry(msm_amd_ctx* ctx, size_t n, uint32_t window_size, uint32_t auto_c, uint32_t* c, uint32_t* W) {
  *c = window_size ? window_size : auto_c;
  if (*c < 4 || *c > 21) return fail(ctx, MSM_AMD_INPUT_ERROR, "table window_size must be 0 (auto) or 4..21");
  *W = kModulusBits / *c + 1;
  if ((size_t)*W * n > 0x7FFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "windows * n must stay below 2^31");
  return MSM_AMD_OK;
}

// The plan of one instance: make_plan and what depends on whether the instance has the machine to itself.
Plan instance_plan(size_t n, uint32_t c, uint32_t table_windows, bool lone, WidthBound width = WidthBound{}) {
  Plan p = make_plan(n, c, table_windows, width);
  if (lone) p.red_group = pick_reduce_group(p);   // (pipelined small instances: 2^16 -6 %, 2^18 +3 % -- not taken)
  p.rb_threads = lone ? 0u : 64u;                 // one wave per bit-subset sum beside a resident accumulate grid (k_reduce.hip)
  // the tile-staged scatter (1024-thread workgroups, 60 VGPRs, 64 KB of LDS) is for a sort that has the machine to
  // itself; beside a resident accumulate grid it is slower than the plain scatter (4 x 2^22 points: 6.15 vs 5.65 ms per MSM)
  if (!lone && !std::getenv("MSM_AMD_TILED")) p.tiled = 0;
  return p;
}

uint32_t auto_table_window(size_t n) {
  // One bucket set serves all windows, so the window can grow until the 2^(c-1) buckets of the window reduction
  // (2 full additions each) cost as much as the mixed additions they save.  Windows whose top digit is narrow are
  // excluded: the n entries of the top window would all fall into its few slots (c = 19 leaves 7 bits for the top
  // window of a 254-bit scalar: 2^20 entries in 128 buckets and in ONE region of the sort).
  uint32_t best = 4;
  double best_cost = 1e300;
  for (uint32_t c = 4; c <= 21; ++c) {
    const uint32_t W = kModulusBits / c + 1;
    const uint32_t top = kModulusBits - (W - 1) * c;          // bits of the top window
    if (top + 6 < c && c > 6) continue;                        // top window concentrated > 64-fold
    if ((size_t)W * n > 0x7FFFFFFFull) continue;
    const double cost = 9.5 * (double)W * (double)n + 27.0 * (double)((size_t)1 << (c - 1)) + 14.0 * (double)W * (double)n / 32.0;
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}
}}  // namespace msm_amd::drv

extern "C" {

uint32_t msm_amd_auto_window_size(size_t n) { return auto_window(n); }
uint32_t msm_amd_auto_window_size_lone(size_t n) { return auto_window_lone(n); }
uint32_t msm_amd_auto_window_size_bounded(size_t n, uint32_t bits, int lone) {
  return auto_window_bounded(n, std::max(1u, std::min(bits, kModulusBits)), lone != 0);
}

uint64_t msm_amd_algorithmic_bytes(size_t n, uint32_t window_size, int accumulate_only) {
  // A(n) = 32n + 72nW + 2*96*totB ; A3(n) = 72nW + 96*totB, with
  // totB = W * (2^c - 1), 64-byte affine bases, 8-byte (bucket, point) pairs, 96-byte buckets.
  const uint64_t c = window_size ? window_size : auto_window(n);
  const uint64_t W = (kModulusBits + c - 1) / c;
  const uint64_t totB = W * ((1ull << c) - 1);
  if (accumulate_only) return 72ull * n * W + 96ull * totB;
  return 32ull * n + 72ull * n * W + 2ull * 96ull * totB;
}

}  // extern "C"
