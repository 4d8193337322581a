// halo2's permuted lookup columns A', S' over BN254 Fr (msm_amd_fr_lookup_permute*): the plan and the bodies shared by the
// kernels (k_permute.hip), the host twin (host_lookup.hip) and the host driver (calls_fr.hip).  Everything here compiles
// for the device and for the host (MSM_HD).
//
// Row order, not value order.  With t[j] the rows of a lookup handle (fr_lookup.hip.h), rep(x) the smallest row equal to x,
// and for one input column f of n records
//     c[j]   = #{ i : rep(f[i]) = j }            (a duplicate row that is not the representative has c = 0)
//     off[j] = sum of c[j'] over j' < j
//     ub[j]  = #{ j' < j : c[j'] = 0 }
//     U      = the rows with c = 0, ascending: row j with c[j] = 0 is U[ub[j]]
// the columns are
//     A'[p] = t[j]                              for off[j] <= p < off[j] + c[j]
//     S'[p] = t[j]                              for p = off[j], c[j] > 0 (a "head")
//     S'[p] = t[U[p - (j - ub[j]) - 1]]         for off[j] < p < off[j] + c[j]: j - ub[j] + 1 heads lie at or before p
// S' needs n = n_rows: then there are as many positions that are no head as there are rows in U.  A' is a permutation of
// the inputs, S' of the table, A'[0] = S'[0], and A'[p] = S'[p] or A'[p] = A'[p - 1] for every p > 0: what halo2's
// verifier asks of the two columns.  halo2's own prover orders A' by ascending field value; that is another arrangement
// of the same multisets which the verifier cannot tell from this one: kPermuteHalo2 below, over a handle whose rows were
// sorted (fr_sort.hip.h).  Every byte is determined by the table and the inputs, not by the order in which atomics land.
//
// Phases, in launch order on one stream (no lane waits for another, every loop has a bound known at launch):
//   count    the probe of k_lookup.hip, counting into per-column counters: counter (v n_rows + j) for column v
//   scan     the exclusive scan of the pairs (c[j], c[j] == 0) over the rows of every column as ONE 64-bit sum -- off in
//            the low word, ub in the high word; both stay below 2^32 -- on the tiles and levels of fr_scan_plan(n_rows,
//            n_vec, tile_log) with 64-bit words for records: L - 1 reductions to the tile totals, the scan of the top level,
//            L - 1 scans downwards, 2 L - 1 launches.  One wave owns a tile of 2^T words (kPermuteTileLog = 11,
//            MSM_AMD_PERMUTE_TILE_LOG lowers it) and walks it 64 words at a time.
//   compact  inside the level-0 scan, which is the one launch that holds c[j] and ub[j] of every row: one lane per row, a
//            row with c = 0 stores j at U[ub[j]]; the same launch folds rows_hit and max_multiplicity into the report
//   fill     one lane per output position p: the owner j = the last row with off[j] <= p by a binary search over off
//            (ceil(log2 n_rows) steps, whatever the multiplicities are), then the stores above.  The lanes read the
//            miss counter of the probe launch and store nothing if it is not zero.
//            MSM_AMD_PERMUTE_FILL=scan finds the owner without the search: the level-0 scan also stores j at owner[off[j]]
//            for every row with c > 0 into n_vec n cleared 32-bit words, an inclusive maximum scan over the positions of
//            every column (fr_permute_owner_plan: the same tiles and levels over n, 2 L' - 1 launches more) spreads each
//            head's row over its group, and the fill reads owner[p].  Measured: DESIGN.md section 8.15.
//
// Workspace of one call in ctx-owned memory (fr_permute_plan): n_vec n_rows 32-bit counters, the 64-byte report record of
// fr_lookup.hip.h, n_vec n_rows pairs, the tile totals of the levels above, n_vec n_rows words of U.
#pragma once
#include "fr_lookup.hip.h"

namespace msm_amd {

constexpr uint32_t kPermuteTileLog = 11;      // 2^11 words per scan tile: two levels up to 2^22 rows
constexpr uint32_t kPermuteMinTileLog = 2;
constexpr uint32_t kPermuteThreads = 256;

struct FrPermutePlan {
  FrScanPlan scan;       // levels over the rows of a column; a record of that plan is one 64-bit pair here
  uint32_t launches;     // kernels of a call that has inputs: the probe, 2 levels - 1 of the scan, the fill
  uint32_t search_steps; // ceil(log2 n_rows): the trip count of the owner search
  uint64_t report_off, pairs_off, totals_off, u_off, bytes;   // the workspace, in bytes; the counters are at 0
};

// n_rows >= 1, n_vec >= 1, n_rows n_vec < 2^32, tile_log: kPermuteMinTileLog .. kPermuteTileLog
inline FrPermutePlan fr_permute_plan(uint64_t n_rows, uint64_t n_vec, uint32_t tile_log) {
  FrPermutePlan p{};
  p.scan = fr_scan_plan(n_rows, n_vec, tile_log);
  p.launches = p.scan.launches + 2;
  while (((uint64_t)1 << p.search_steps) < n_rows) ++p.search_steps;
  const uint64_t cells = n_rows * n_vec;
  p.report_off = (cells * 4 + 15) & ~(uint64_t)15;
  p.pairs_off = p.report_off + kLookupReportWords * 8;
  p.totals_off = p.pairs_off + cells * 8;
  p.u_off = p.totals_off + p.scan.records * 8;
  p.bytes = p.u_off + cells * 4;
  return p;
}

// how the fill finds the owner of a position (MSM_AMD_PERMUTE_FILL): the binary search, or the heads scattered and spread
// by a maximum scan
enum { kPermuteFillSearch = 0, kPermuteFillScan = 1 };
constexpr int kPermuteFillDefault = kPermuteFillSearch;   // measured: DESIGN.md section 8.15

// kPermuteFillScan: the owner words of every position (level 0) and of the tiles above, behind the workspace of
// fr_permute_plan; a record of the scan plan is one 32-bit word here
struct FrPermuteOwnerPlan {
  FrScanPlan scan;
  uint64_t owner_off, totals_off, bytes;   // from the start of the workspace
};
inline FrPermuteOwnerPlan fr_permute_owner_plan(const FrPermutePlan& p, uint64_t n, uint64_t n_vec, uint32_t tile_log) {
  FrPermuteOwnerPlan o{};
  o.scan = fr_scan_plan(n, n_vec, tile_log);
  o.owner_off = (p.bytes + 15) & ~(uint64_t)15;
  o.totals_off = o.owner_off + n * n_vec * 4;
  o.bytes = o.totals_off + o.scan.records * 4;
  return o;
}

// the pair of a counter: c in the low word, (c == 0) in the high word
MSM_HD uint64_t fr_permute_pair(uint32_t c) { return (uint64_t)c | ((uint64_t)(c == 0) << 32); }
MSM_HD uint32_t fr_permute_off(uint64_t pair) { return (uint32_t)pair; }
MSM_HD uint32_t fr_permute_ub(uint64_t pair) { return (uint32_t)(pair >> 32); }

// The owner of position p: the last row j < n_rows with off[j] <= p, over the scanned pairs of one column.  off[0] = 0, so
// row 0 qualifies for every p; `steps` >= ceil(log2 n_rows) halvings leave one row.  If p < the sum of the counters the
// owner has c > 0: a row with c = 0 shares its off with its successor.
MSM_HD uint32_t fr_permute_owner(const uint64_t* pairs, uint32_t n_rows, uint32_t steps, uint32_t p) {
  uint32_t lo = 0, hi = n_rows;   // off[lo] <= p, and off[hi] > p or hi == n_rows
  NTT_NO_UNROLL for (uint32_t s = 0; s < steps; ++s) {
    if (hi - lo <= 1) break;
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (fr_permute_off(pairs[mid]) <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// Where S'[p] comes from, p owned by row j with the scanned pair `pair`: the head of a group takes the row itself, every
// other position the next unused row.  Returns true for a head; else *k is the index into U.
MSM_HD bool fr_permute_head(uint32_t p, uint32_t j, uint64_t pair, uint32_t* k) {
  if (p == fr_permute_off(pair)) return true;
  *k = p - (j - fr_permute_ub(pair)) - 1u;
  return false;
}

// The two arrangements (MSM_AMD_PERMUTE_*).  Over a handle whose rows are sorted by value (msm_amd_fr_lookup_build_sorted:
// row k is sorted position k, equal values in their input order) the columns above ARE those of halo2's
// permute_expression_pair but for the gaps: A' is the input column ascending, the heads are the positions where A' changes,
// and U lists the leftover table values ascending, duplicates included.  halo2 fills the positions that are no head from
// the LAST one downwards (repeated_input_rows.pop()), so the g-th of them, ascending, holds U[G - 1 - g], G = |U|, where the
// row-order arrangement holds U[g].
enum { kPermuteRows = 0, kPermuteHalo2 = 1 };
// G of a column from its last scanned pair and that row's own counter
MSM_HD uint32_t fr_permute_unused_rows(uint64_t last_pair, uint32_t last_counter) {
  return fr_permute_ub(last_pair) + (uint32_t)(last_counter == 0);
}
// the index into U of the g-th position that is no head, g < unused_rows
MSM_HD uint32_t fr_permute_gap(int arrangement, uint32_t g, uint32_t unused_rows) {
  return arrangement == kPermuteHalo2 ? unused_rows - 1u - g : g;
}

}  // namespace msm_amd
