// Vectors over BN254 Fr (msm_amd_fr_map*, msm_amd_fr_batch_inverse*, msm_amd_fr_prefix_product*; the polynomial calls
// msm_amd_fr_poly_*, msm_amd_fr_lincomb* run on the same scan plan, see launch_fr.h): the bodies shared by
// the kernels (k_fr.hip), the host twin (host_fr.hip) and the host driver (msm_host.hip).  Everything here compiles for
// the device and for the host (MSM_HD).  Records are read with ntt_load and written with ntt_store (ntt.hip.h): any
// 256-bit input is taken mod r, every output is the fully reduced residue in the layout of the input.
//
// Scan plan (fr_scan_plan).  A tile is 2^T consecutive records of one vector (kFrTileLog = 9, MSM_AMD_FR_TILE_LOG lowers
// it), ceil(n / 2^T) tiles per vector.  Level 0 is the caller's data, level k + 1 holds one record per tile of level k:
// the tile's product.  The levels end at the first one that is a single tile per vector.  With L levels a scan is
//     L - 1 reductions  (level k -> the totals of level k + 1, k = 0 .. L - 2)
//     1 scan            of level L - 1 in place (exclusive: a total becomes the product of the tiles before it)
//     L - 1 scans       of level k, k = L - 2 .. 0, every tile starting from its record of level k + 1
// in stream order: 2 L - 1 launches, and sum_{k >= 1} n_vec len_k records of ctx-owned memory.  L = 1 up to n = 2^T, 2 up
// to 2^(2T), 3 beyond.  No launch waits on another workgroup.
//
// Batch inversion (one inversion per call).  With zeros replaced by one, t_b = the product of tile b, P_b / S_b the
// inclusive prefix / suffix products of the t_b and T = P_last:  (t_b)^-1 = T^-1 P_(b-1) S_(b+1).  The tiles of the
// inversion are 2^min(T, kFrInvTileLog) records: its last kernel keeps two records per element in LDS.
//
// Tile sizes.  One wave owns a tile and keeps it in LDS, 32 bytes per record, so the tile decides how many waves share a CU's
// 160 KiB: 2^10 records leave one wave per SIMD, 2^9 two, 2^8 four -- and a smaller tile pays the six products of a
// scan over the lanes more often.  Measured at 2^24 records: the scan is fastest at 2^9, the inversion
// (two LDS images) at 2^8.
#pragma once
#include "ntt.hip.h"

namespace msm_amd {

constexpr uint32_t kFrTileLog = 9;         // 2^9 records per scan tile: 8 per lane of one wave, 18 KiB of LDS
constexpr uint32_t kFrInvTileLog = 8;      // 2^8 records per tile of the inversion: 4 per lane, two LDS images of 10 KiB
constexpr uint32_t kFrMinTileLog = 2;
constexpr uint32_t kFrWave = 64;           // one wave per tile
constexpr uint32_t kFrMapThreads = 256;
constexpr uint32_t kFrMaxLevels = 16;      // n < 2^32 at tiles of 4
constexpr int kFrRaw = -1;                 // layout of the tile totals: reduced Montgomery residues, no conversion
enum { kFrAdd = 0, kFrSub, kFrMul, kFrScale, kFrAxpy, kFrMulsubScale, kFrOps };
constexpr int kFrShift = kFrOps;           // a + k (msm_amd_fr_shift*): a kernel of the map, no op of msm_amd_fr_map (it reads 0)
constexpr int kFrInclusive = 0, kFrExclusive = 1;
constexpr unsigned kFrReadsA = 1, kFrReadsB = 2, kFrReadsC = 4, kFrReadsK = 8;

// what an op reads: a mask of kFrReads*; 0 for an unknown op
MSM_HD constexpr unsigned fr_op_reads(int op) {
  switch (op) {
    case kFrAdd: case kFrSub: case kFrMul: return kFrReadsA | kFrReadsB;
    case kFrScale: return kFrReadsA | kFrReadsK;
    case kFrAxpy: return kFrReadsA | kFrReadsB | kFrReadsK;
    case kFrMulsubScale: return kFrReadsA | kFrReadsB | kFrReadsC | kFrReadsK;
    default: return 0;
  }
}

// One element of a map; everything Montgomery and reduced.  Operands the op does not read are ignored.
template <int OP>
MSM_HD u256 fr_map_op(const u256& k, const u256& a, const u256& b, const u256& c) {
  if (OP == kFrAdd) return Fr::add(a, b);
  if (OP == kFrSub) return Fr::sub(a, b);
  if (OP == kFrMul) return Fr::mul(a, b);
  if (OP == kFrScale) return Fr::mul(k, a);
  if (OP == kFrAxpy) return Fr::add(a, Fr::mul(k, b));
  if (OP == kFrShift) return Fr::add(a, k);
  return Fr::mul(k, Fr::sub(Fr::mul(a, b), c));
}

// The monoid of a scan: the products of msm_amd_fr_prefix_product*, or (SUM) the sums of msm_amd_fr_prefix_sum*
template <bool SUM>
MSM_HD u256 fr_scan_unit() { return SUM ? u256_zero() : Fr::one(); }
template <bool SUM>
MSM_HD u256 fr_scan_op(const u256& a, const u256& b) { return SUM ? Fr::add(a, b) : Fr::mul(a, b); }

MSM_HD u256 fr_load(int layout, const u256& rec) { return layout == kFrRaw ? rec : ntt_load(layout, rec.v); }
MSM_HD u256 fr_store(int layout, const u256& x) {
  if (layout == kFrRaw) return x;
  u256 r;
  ntt_store(layout, x, r.v);
  return r;
}
MSM_HD u256 fr_select(bool take_a, const u256& a, const u256& b) {
  u256 r;
  MSM_UNROLL for (int i = 0; i < 8; ++i) r.v[i] = take_a ? a.v[i] : b.v[i];
  return r;
}

struct FrScanPlan {
  uint32_t levels;                    // >= 1
  uint32_t launches;                  // 2 levels - 1
  uint64_t len[kFrMaxLevels];         // records per vector at level k
  uint64_t tiles[kFrMaxLevels];       // tiles per vector at level k
  uint64_t offset[kFrMaxLevels];      // level k >= 1: first record of its totals in the workspace
  uint64_t records;                   // the workspace: all totals of all vectors
};

// n >= 1, n_vec >= 1, n n_vec < 2^32, tile_log: kFrMinTileLog .. kFrTileLog
inline FrScanPlan fr_scan_plan(uint64_t n, uint64_t n_vec, uint32_t tile_log) {
  FrScanPlan p{};
  uint64_t len = n;
  for (;;) {
    const uint64_t tiles = (len + ((uint64_t)1 << tile_log) - 1) >> tile_log;
    p.len[p.levels] = len, p.tiles[p.levels] = tiles;
    p.offset[p.levels] = p.records;
    if (p.levels) p.records += len * n_vec;
    ++p.levels;
    if (tiles <= 1) break;
    len = tiles;
  }
  p.launches = 2 * p.levels - 1;
  return p;
}

// Several points per pass (msm_amd_fr_poly_eval_points, msm_amd_fr_poly_div_points; launch_fr.h).  With pairwise distinct
// z_0 .. z_(k-1), w_j = 1 / prod_(m != j) (z_j - z_m) and s^(j)_i = sum_(t >= i) c_t z_j^(t - i), the suffix sums of the
// division by X - z_j, the floor quotient of p by prod_j (X - z_j) is
//     q_i = sum_j w_j s^(j)_(i+1)                                       (partial fractions of 1 / prod_j (X - z_j))
// and s^(j)_0 = p(z_j).  sum_j w_j z_j^m = 0 for m < k - 1: the top min(k, n) records come out as exact zeros, and with
// m = 0 the sum is sum_(j < k-1) w_j (s^(j) - s^(k-1)), k - 1 products per record.  The k scans run side by side on the
// scan plan of one point: level 0 reads the caller's tile once and carries k running values through it, the levels above
// hold k copies of the single-point totals, point-major, and run in one launch per level over (point, vector, tile).
constexpr uint32_t kFrPolyMaxPoints = 8;
// The arguments of both kernels, by value: the powers of every point's level point x_j = z_j^(2^(T level)) and the weights
struct FrPolyPointsArgs {
  const uint32_t* src;
  uint32_t* dst;               // scan
  const uint32_t* carry;       // scan: the level above; null: every carry is zero
  uint32_t* totals;            // reduce: one raw record per point and tile; scan: s_0 of every tile, raw (optional)
  uint64_t len, tiles;         // records and tiles per vector
  uint64_t src_stride;         // records between the copies of src / dst of two points (0 at level 0: one src for all)
  uint64_t tot_stride;         // records between the carry / totals of two points
  uint32_t tile_log;
  int layout, level0;          // level0 (scan): slot i takes sum_j w_j s^(j)_(i+1); else s_i of the block's one point
  u256 z[kFrPolyMaxPoints];         // x_j
  u256 step[kFrPolyMaxPoints][7];   // reduce: x_j^(2^s), s < 6, and x_j^64; scan: x_j^(per 2^s), s < 6
  u256 w[kFrPolyMaxPoints];         // level 0 of a division
};
static_assert(sizeof(FrPolyPointsArgs) < 4096, "the kernel arguments stay under 4 KiB");

// The workspace of one inversion of n records, in records: the tile products t, P with one record more (the zero
// count, so that T = P_last and the count leave in one copy), S, and the workspace of the scans of t.
struct FrInvPlan {
  uint32_t tile_log;
  uint64_t tiles, t_off, p_off, s_off, scan_off, records;
};
inline FrInvPlan fr_inv_plan(uint64_t n, uint32_t tile_log) {
  FrInvPlan p{};
  p.tile_log = tile_log < kFrInvTileLog ? tile_log : kFrInvTileLog;
  p.tiles = (n + ((uint64_t)1 << p.tile_log) - 1) >> p.tile_log;
  p.t_off = 0, p.p_off = p.tiles, p.s_off = p.p_off + p.tiles + 1, p.scan_off = p.s_off + p.tiles;
  p.records = p.scan_off + fr_scan_plan(p.tiles, 1, tile_log).records;
  return p;
}

}  // namespace msm_amd
