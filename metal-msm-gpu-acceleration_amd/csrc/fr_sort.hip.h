// Sorting columns of BN254 Fr records by canonical value (msm_amd_fr_sort, msm_amd_host_fr_sort): the plan and the bodies
// shared by the kernels (k_fr_sort.hip), the host twin (host_fr_sort.hip) and the host driver (calls_fr.hip).  Everything here
// compiles for the device and for the host (MSM_HD).
//
// The key of a record is its residue in [0, r) as 32 little-endian bytes (fr_sort_key): halo2curves' Ord for Fr compares
// to_repr() from the top byte down, which is the order of that residue as an integer.  It is neither the Montgomery words
// nor the caller's unreduced word.  The sort is stable: records equal mod r keep their input order, so the permutation is
// unique and no byte of any output depends on how the work was cut.
//
// Phases of a call, in launch order on one stream (no lane waits for another workgroup, every loop bound is known at launch):
//   keys     one lane per record of the call: load, reduce, leave Montgomery form, store the key in ctx-owned memory, and fold
//            the digit mask: bit d is set iff byte d of some key differs from byte d of the key of record 0 (the first lane
//            of every workgroup forms that key and shares it through LDS: no launch and no device memory of its own).
//            Per-wave OR, one atomic OR per wave.
//   (wait)   the mask comes back in the call's one bounded wait; a pass runs only for a set bit.  Lookup columns are mostly
//            small values: 2 to 3 passes instead of 32.  The mask chooses the passes, never a byte of the output: a byte
//            that is equal in every key does not order any two of them.
//   sort     column by column, least significant digit first, 8 bits per pass.  For every 32-bit word w of the key with
//            set mask bits, lowest first, one gather launch builds the pairs (word w of key[perm[i]], perm[i]) -- perm is
//            the identity before the first one -- and the set bytes of that word take one pass each over the 8-byte pairs:
//            histogram per tile, row scan, ballot-ranked scatter, on tiles of 4096 pairs of which each of the four waves owns
//            a contiguous quarter (the scheme of k_stage.hip's radix kernels).  At most eight random gathers per column.
//   gather   out[k] = the record of key[perm[k]] in the caller's layout, perm_out[k] = perm[k].  A mask of 0 needs no pairs:
//            the identity.  Every index read from the pairs is checked against n before it addresses memory.
//
// Workspace of one call in ctx-owned memory (fr_sort_plan): the 64-byte record with the mask in its first word, the keys of
// every column, two arrays of n pairs and the tile histograms of one column (the columns follow each other on the stream).
#pragma once
#include "fr_vec.hip.h"

namespace msm_amd {

constexpr uint32_t kSortThreads = 256;
constexpr uint32_t kSortItems = 16;                          // pairs per lane of a tile
constexpr uint32_t kSortTile = kSortThreads * kSortItems;    // 4096 pairs: a quarter of 1024 per wave
constexpr uint32_t kSortRecordBytes = 64;                    // the call's record: the mask, then zeros

struct FrSortPlan {
  uint32_t passes;      // 8-bit passes over one column: popcount(mask)
  uint32_t words;       // 32-bit words of the key with set mask bits: gather launches of one column
  uint32_t launches;    // kernels of the whole call: the keys, per column `words` gathers, 3 per pass, the final gather
  uint64_t tiles;       // tiles of a pass
  uint64_t keys_off, pairs_off, hist_off, bytes;   // the workspace, in bytes; the record is at 0
};

// n >= 1, n_vec >= 1, n n_vec < 2^32
inline FrSortPlan fr_sort_plan(uint64_t n, uint64_t n_vec, uint32_t mask) {
  FrSortPlan p{};
  for (uint32_t w = 0; w < 8; ++w) {
    const uint32_t bits = (mask >> (4 * w)) & 0xFu;
    p.words += bits != 0;
    for (uint32_t b = 0; b < 4; ++b) p.passes += (bits >> b) & 1u;
  }
  p.tiles = (n + kSortTile - 1) / kSortTile;
  p.launches = (uint32_t)(1 + n_vec * (p.words + 3 * (uint64_t)p.passes + 1));
  p.keys_off = kSortRecordBytes;
  p.pairs_off = p.keys_off + n * n_vec * 32;
  p.hist_off = p.pairs_off + 2 * n * 8;
  p.bytes = p.hist_off + 256 * (p.tiles + 1) * 4;
  return p;
}

// the canonical key of a record of the caller: the residue, little-endian words
MSM_HD u256 fr_sort_key(int layout, const u256& rec) {
  u256 k = rec;
  NTT_NO_UNROLL for (int i = 0; i < 5; ++i) k = Fr::reduce_once(k);   // any 256-bit word mod r, as ntt_load
  return layout == kNttCanonLe ? k : Fr::from_mont(k);
}
// the record of a key in the caller's layout, fully reduced
MSM_HD u256 fr_sort_record(int layout, const u256& key) { return layout == kNttCanonLe ? key : Fr::to_mont(key); }

// bit d: byte d of a differs from byte d of b
MSM_HD uint32_t fr_sort_diff(const u256& a, const u256& b) {
  uint32_t m = 0;
  MSM_UNROLL for (int w = 0; w < 8; ++w) {
    const uint32_t x = a.v[w] ^ b.v[w];
    MSM_UNROLL for (int k = 0; k < 4; ++k) m |= (uint32_t)(((x >> (8 * k)) & 0xFFu) != 0) << (4 * w + k);
  }
  return m;
}

// a < b as integers
MSM_HD bool fr_sort_less(const u256& a, const u256& b) {
  for (int w = 7; w >= 0; --w)
    if (a.v[w] != b.v[w]) return a.v[w] < b.v[w];
  return false;
}

}  // namespace msm_amd
