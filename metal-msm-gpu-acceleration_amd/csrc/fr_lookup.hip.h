// Lookup tables over BN254 Fr (msm_amd_fr_lookup_*): the hash, the plan and the probe bodies shared by the kernels
// (k_lookup.hip), the host twin (host_lookup.hip) and the host driver (calls_fr.hip).  Everything here compiles for the
// device and for the host (MSM_HD).
//
// A table is one column of n_rows records.  The handle keeps them as reduced Montgomery residues (ntt_load of the
// caller's layout: equal mod r means equal words) and an open-addressing index over them:
//     capacity   the power of two >= 2 n_rows (never below 2): the load is at most 1/2
//     slot       one 32-bit word: a row index, or kLookupEmpty
//     home       capacity - 1 - (hash & (2^min(b, log2 capacity) - 1)), b = MSM_AMD_LOOKUP_HASH_BITS (default: all): homes
//                are taken from the top of the slot array, the probe walks upwards and wraps to slot 0, so that with few
//                hash bits the chains cross the end of the array (b = 0: one chain from the last slot)
//     hash       MurmurHash3 (x86, 32 bits) over the eight words of the residue
// Rows that are equal share one slot, and the slot ends up holding the smallest of their indices whatever the order of
// arrival: an empty slot is claimed by compare-and-swap, an occupant with equal words is lowered by an atomic minimum, a
// lost compare-and-swap reads the same slot again (it is occupied for good) and goes on.  A slot never changes the class
// of equal rows it stands for, so every row of a class stops at the same slot.  Every loop ends after `capacity` slots;
// one that gets there sets the error word.  No lane waits for another.
//
// Image of a handle in device memory (fr_lookup_plan): the rows, the slots, and eight 32-bit words of statistics
// (kLookupDistinct: claimed slots, kLookupLongest: most slots one insert looked at, kLookupError).
//
// A multiplicities call counts in ctx-owned memory (fr_lookup_work): n_rows 32-bit counters, then the 64-byte record
// { n_missing, first_missing, rows_hit, max_multiplicity, error, 0, 0, 0 } of 64-bit words, then (host form) the staging
// of the row indices.
#pragma once
#include "fr_vec.hip.h"

namespace msm_amd {

constexpr uint32_t kLookupEmpty = 0xFFFFFFFFu;
constexpr uint32_t kLookupAllBits = 32;
constexpr uint32_t kLookupThreads = 256;
constexpr uint32_t kLookupBlockThreads = 1024;   // the probe launch of kLookupCountBlock: 16 waves fold their largest groups
enum { kLookupDistinct = 0, kLookupLongest, kLookupError, kLookupStatWords = 8 };
enum { kLookupStrict = 0, kLookupCountMissing = 1 };
enum { kLookupMissing = 0, kLookupFirstMissing, kLookupRowsHit, kLookupMaxMult, kLookupReportError, kLookupReportWords = 8 };
// how the hits are counted (MSM_AMD_LOOKUP_COUNT): one atomic per lane, one per distinct row of a wave, or that with the
// largest group of each of a workgroup's 16 waves folded through LDS first
enum { kLookupCountLane = 0, kLookupCountWave = 1, kLookupCountBlock = 2 };
constexpr int kLookupCountDefault = kLookupCountBlock;   // measured: DESIGN.md section 8.14

struct FrLookupPlan {
  uint32_t cap_log, home_bits;           // home_bits = min(hash_bits, cap_log)
  uint64_t capacity;
  uint64_t rows_off, slots_off, stats_off, bytes;   // the image, in bytes
};

// 1 <= n_rows < 2^31
MSM_HD FrLookupPlan fr_lookup_plan(uint64_t n_rows, uint32_t hash_bits) {
  FrLookupPlan p{};
  p.cap_log = 1;
  while (((uint64_t)1 << p.cap_log) < 2 * n_rows) ++p.cap_log;
  p.capacity = (uint64_t)1 << p.cap_log;
  p.home_bits = hash_bits < p.cap_log ? hash_bits : p.cap_log;
  p.rows_off = 0;
  p.slots_off = n_rows * 32;
  p.stats_off = p.slots_off + p.capacity * 4;
  p.bytes = p.stats_off + kLookupStatWords * 4;
  return p;
}

struct FrLookupWork {
  uint64_t report_off, idx_off, bytes;   // the counters are at 0
};
MSM_HD FrLookupWork fr_lookup_work(uint64_t n_rows, uint64_t staged_idx) {
  FrLookupWork w{};
  w.report_off = (n_rows * 4 + 15) & ~(uint64_t)15;
  w.idx_off = w.report_off + kLookupReportWords * 8;
  w.bytes = w.idx_off + staged_idx * 4;
  return w;
}

MSM_HD uint32_t fr_lookup_rotl(uint32_t x, uint32_t s) { return (x << s) | (x >> (32u - s)); }

// MurmurHash3_x86_32 of the 32 bytes of a residue, seed 0
MSM_HD uint32_t fr_lookup_hash(const u256& x) {
  uint32_t h = 0;
  MSM_UNROLL for (int w = 0; w < 8; ++w) {
    uint32_t k = x.v[w] * 0xCC9E2D51u;
    k = fr_lookup_rotl(k, 15) * 0x1B873593u;
    h = fr_lookup_rotl(h ^ k, 13) * 5u + 0xE6546B64u;
  }
  h ^= 32u;
  h ^= h >> 16, h *= 0x85EBCA6Bu;
  h ^= h >> 13, h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

MSM_HD uint32_t fr_lookup_home(const FrLookupPlan& p, const u256& x) {
  const uint32_t keep = p.home_bits >= 32u ? 0xFFFFFFFFu : ((1u << p.home_bits) - 1u);
  return (uint32_t)(p.capacity - 1u) - (fr_lookup_hash(x) & keep);
}

MSM_HD bool fr_lookup_same(const u256& a, const u256& b) {
  uint32_t d = 0;
  MSM_UNROLL for (int w = 0; w < 8; ++w) d |= a.v[w] ^ b.v[w];
  return d == 0;
}

// Row j (value x = row(j)) into the index.  Mem: load(slots, at) -> word, cas(slots, at, expect, value) -> the word before,
// lower(slots, at, value): atomic minimum, row(i) -> the residue of row i.  Returns the number of slots looked at (0: the
// capacity ran out, which cannot happen at load <= 1/2); *claimed is set when this row took an empty slot.
template <class Mem>
MSM_HD uint32_t fr_lookup_insert(const FrLookupPlan& p, Mem& mem, uint32_t j, const u256& x, bool* claimed) {
  const uint32_t mask = (uint32_t)(p.capacity - 1u);
  uint32_t at = fr_lookup_home(p, x);
  *claimed = false;
  NTT_NO_UNROLL for (uint64_t step = 1; step <= p.capacity; ++step, at = (at + 1u) & mask) {
    uint32_t cur = mem.load(at);
    if (cur == kLookupEmpty) {
      cur = mem.cas(at, kLookupEmpty, j);
      if (cur == kLookupEmpty) {
        *claimed = true;
        return (uint32_t)step;
      }
    }
    // occupied for good; the occupant may still be lowered, to a row of the same words
    if (fr_lookup_same(mem.row(cur), x)) {
      if (j < cur) mem.lower(at, j);
      return (uint32_t)step;
    }
  }
  return 0;
}

// The representative of x in a finished index, or kLookupEmpty.  *exhausted: the capacity ran out.
template <class Mem>
MSM_HD uint32_t fr_lookup_find(const FrLookupPlan& p, Mem& mem, const u256& x, bool* exhausted) {
  const uint32_t mask = (uint32_t)(p.capacity - 1u);
  uint32_t at = fr_lookup_home(p, x);
  *exhausted = false;
  NTT_NO_UNROLL for (uint64_t step = 0; step < p.capacity; ++step, at = (at + 1u) & mask) {
    const uint32_t cur = mem.load(at);
    if (cur == kLookupEmpty) return kLookupEmpty;
    if (fr_lookup_same(mem.row(cur), x)) return cur;
  }
  *exhausted = true;
  return kLookupEmpty;
}

// a count c < 2^32 as a reduced Montgomery residue
MSM_HD u256 fr_lookup_count(uint32_t c) {
  u256 x = u256_zero();
  x.v[0] = c;
  return Fr::to_mont(x);
}

}  // namespace msm_amd
