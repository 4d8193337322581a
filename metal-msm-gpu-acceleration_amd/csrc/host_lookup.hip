// Host twin of the lookup calls over Fr (no ctx, no GPU): the index of fr_lookup.hip.h built row by row in row order, the
// inputs split over the host threads, each thread probing the finished index and counting in the shared 32-bit counters;
// and the argument checks and knobs the twin shares with the host driver (calls_fr.hip).  Representatives, counts, indices
// and the report are unique, so neither the hash nor the way the twin cuts the work shows in any byte.  The twin of the
// permuted columns (fr_permute.hip.h) counts per column in the same way.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_fr.h"

namespace msm_amd {

static_assert(kLookupStrict == MSM_AMD_LOOKUP_STRICT && kLookupCountMissing == MSM_AMD_LOOKUP_COUNT_MISSING, "modes");
static_assert(kPermuteRows == MSM_AMD_PERMUTE_ROWS && kPermuteHalo2 == MSM_AMD_PERMUTE_HALO2, "arrangements");

uint32_t fr_lookup_hash_bits_knob() {
  if (const char* e = std::getenv("MSM_AMD_LOOKUP_HASH_BITS"))
    return (uint32_t)std::max(0, std::min((int)kLookupAllBits, std::atoi(e)));
  return kLookupAllBits;
}

int fr_lookup_count_knob() {
  if (const char* e = std::getenv("MSM_AMD_LOOKUP_COUNT")) {
    if (std::strcmp(e, "lane") == 0) return kLookupCountLane;
    if (std::strcmp(e, "wave") == 0) return kLookupCountWave;
    if (std::strcmp(e, "block") == 0) return kLookupCountBlock;
  }
  return kLookupCountDefault;
}

const char* fr_lookup_table_check(int scalar_layout, const void* table, uint64_t n_rows, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (n_rows == 0) return "n_rows must be at least 1";
  if (n_rows >> 31) return "n_rows >= 2^31";
  if (!table) return "null table";
  if (device && ((uintptr_t)table & 15u)) return "device buffers must be 16-byte aligned";
  return nullptr;
}

const char* fr_lookup_call_check(int scalar_layout, int on_missing, uint64_t n_rows, const void* in, uint64_t n, uint64_t n_vec,
                                 const void* m_out, const uint32_t* idx_out, const uint64_t* report, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (on_missing != kLookupStrict && on_missing != kLookupCountMissing)
    return "on_missing must be MSM_AMD_LOOKUP_STRICT or MSM_AMD_LOOKUP_COUNT_MISSING";
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (!m_out || !report) return "null m_out or report";
  if (device && ((uintptr_t)m_out & 15u)) return "device buffers must be 16-byte aligned";
  if (n == 0 || n_vec == 0) return nullptr;
  if (!in) return "null pointer with n > 0";
  if (device && ((uintptr_t)in & 15u)) return "device buffers must be 16-byte aligned";
  if (device && ((uintptr_t)idx_out & 3u)) return "d_idx_out must be 4-byte aligned";
  const uintptr_t m = (uintptr_t)m_out, a = (uintptr_t)in, x = (uintptr_t)idx_out;
  const uint64_t m_bytes = n_rows * 32, in_bytes = n * n_vec * 32, idx_bytes = n * n_vec * 4;
  if (m < a + in_bytes && a < m + m_bytes) return "m_out must not overlap the inputs";
  if (idx_out && ((x < a + in_bytes && a < x + idx_bytes) || (x < m + m_bytes && m < x + idx_bytes)))
    return "idx_out must not overlap the inputs or m_out";
  return nullptr;
}

uint32_t fr_permute_tile_log_knob() {
  if (const char* e = std::getenv("MSM_AMD_PERMUTE_TILE_LOG"))
    return (uint32_t)std::max((int)kPermuteMinTileLog, std::min((int)kPermuteTileLog, std::atoi(e)));
  return kPermuteTileLog;
}

int fr_permute_fill_knob() {
  if (const char* e = std::getenv("MSM_AMD_PERMUTE_FILL")) {
    if (std::strcmp(e, "search") == 0) return kPermuteFillSearch;
    if (std::strcmp(e, "scan") == 0) return kPermuteFillScan;
  }
  return kPermuteFillDefault;
}

const char* fr_permute_call_check(int scalar_layout, uint64_t n_rows, const void* in, uint64_t n, uint64_t n_vec,
                                  const void* a_out, const void* s_out, const uint64_t* report) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (!report) return "null report";
  if (!a_out && !s_out) return "a_out or s_out must be given";
  if (n == 0 || n_vec == 0) return nullptr;
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if ((n_rows * n_vec) >> 32) return "n_rows * n_vec >= 2^32";
  if (!in) return "null pointer with n > 0";
  if (s_out && n != n_rows) return "s_out needs n == n_rows";
  const uint64_t bytes = n * n_vec * 32;
  const uintptr_t f = (uintptr_t)in, a = (uintptr_t)a_out, s = (uintptr_t)s_out;
  auto meet = [&](uintptr_t x, uintptr_t y) { return x < y + bytes && y < x + bytes; };
  if (a_out && a != f && meet(a, f)) return "a_out must be the inputs themselves or not overlap them";
  if (s_out && meet(s, f)) return "s_out must not overlap the inputs";
  if (a_out && s_out && meet(a, s)) return "a_out and s_out must not overlap";
  return nullptr;
}

namespace {

u256 host_get(int layout, const uint8_t* base, size_t i) {
  uint32_t rec[8];
  std::memcpy(rec, base + i * 32, 32);
  return ntt_load(layout, rec);
}
void host_put(int layout, uint8_t* base, size_t i, const u256& x) {
  uint32_t rec[8];
  ntt_store(layout, x, rec);
  std::memcpy(base + i * 32, rec, 32);
}

// the index in host memory: built by one thread, then read by many
struct HostMem {
  const u256* rows;
  uint32_t* slots;
  uint32_t load(uint32_t at) { return slots[at]; }
  uint32_t cas(uint32_t at, uint32_t expect, uint32_t value) {
    const uint32_t before = slots[at];
    if (before == expect) slots[at] = value;
    return before;
  }
  void lower(uint32_t at, uint32_t value) { slots[at] = std::min(slots[at], value); }
  u256 row(uint32_t i) { return rows[i]; }
};

// the residues of a table and the index over them, built row by row in row order
struct HostIndex {
  FrLookupPlan plan;
  std::vector<u256> rows;
  std::vector<uint32_t> slots;
  bool build(int layout, const uint8_t* table, size_t n_rows, int threads) {
    plan = fr_lookup_plan(n_rows, fr_lookup_hash_bits_knob());
    rows.resize(n_rows);
    for_ranges(worker_count(threads, n_rows), n_rows, [&](unsigned, size_t lo, size_t hi) {
      for (size_t j = lo; j < hi; ++j) rows[j] = host_get(layout, table, j);
    });
    slots.assign(plan.capacity, kLookupEmpty);
    HostMem mem{rows.data(), slots.data()};
    for (size_t j = 0; j < n_rows; ++j) {
      bool claimed;
      if (!fr_lookup_insert(plan, mem, (uint32_t)j, rows[j], &claimed)) return false;
    }
    return true;
  }
};

}  // namespace

int host_fr_lookup_multiplicities(int layout, int on_missing, const void* table_v, size_t n_rows, const void* in_v, size_t n,
                                  size_t n_vec, int threads, void* m_out_v, uint32_t* idx_out, uint64_t report[4]) {
  if (fr_lookup_table_check(layout, table_v, n_rows, false) ||
      fr_lookup_call_check(layout, on_missing, n_rows, in_v, n, n_vec, m_out_v, idx_out, report, false))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t *table = (const uint8_t*)table_v, *in = (const uint8_t*)in_v;
  uint8_t* m_out = (uint8_t*)m_out_v;
  const size_t total = n * n_vec;
  report[0] = report[1] = report[2] = report[3] = 0;
  if (total == 0) {
    for (size_t j = 0; j < n_rows; ++j) host_put(layout, m_out, j, u256_zero());
    return MSM_AMD_OK;
  }
  HostIndex index;
  if (!index.build(layout, table, n_rows, threads)) return MSM_AMD_PIPELINE_ERROR;
  const FrLookupPlan& plan = index.plan;
  const std::vector<u256>& rows = index.rows;
  std::vector<uint32_t>& slots = index.slots;
  std::vector<uint32_t> counters(n_rows, 0);
  const unsigned T = worker_count(threads, total);
  std::vector<uint64_t> missing(T, 0), first(T, ~(uint64_t)0);
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    HostMem probe{rows.data(), slots.data()};
    for (size_t i = lo; i < hi; ++i) {
      bool exhausted;
      const uint32_t idx = fr_lookup_find(plan, probe, host_get(layout, in, i), &exhausted);
      if (idx_out) idx_out[i] = idx;
      if (idx == kLookupEmpty) {
        if (!missing[t]++) first[t] = i;
      } else {
        __atomic_fetch_add(&counters[idx], 1u, __ATOMIC_RELAXED);
      }
    }
  });
  report[1] = ~(uint64_t)0;
  for (unsigned t = 0; t < T; ++t) report[0] += missing[t], report[1] = std::min(report[1], first[t]);
  for (size_t j = 0; j < n_rows; ++j) report[2] += counters[j] != 0, report[3] = std::max<uint64_t>(report[3], counters[j]);
  if (on_missing == kLookupStrict && report[0]) return MSM_AMD_INPUT_ERROR;
  for_ranges(worker_count(threads, n_rows), n_rows, [&](unsigned, size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; ++j) host_put(layout, m_out, j, fr_lookup_count(counters[j]));
  });
  return MSM_AMD_OK;
}

// The columns of fr_permute.hip.h, straight from the definition: every input is looked up before anything is written (a_out
// may be the inputs), the counters are scanned by one thread, the rows of a column are filled by many.  kPermuteHalo2: the
// twin sorts the table itself (host_fr_sort: what msm_amd_fr_lookup_build_sorted leaves in a handle) and fills the gaps from
// the far end of the unused rows.
int host_fr_lookup_permute(int layout, int arrangement, const void* table_v, size_t n_rows, const void* in_v, size_t n,
                           size_t n_vec, int threads, void* a_out_v, void* s_out_v, uint64_t report[4]) {
  if ((arrangement != kPermuteRows && arrangement != kPermuteHalo2) || fr_lookup_table_check(layout, table_v, n_rows, false) ||
      fr_permute_call_check(layout, n_rows, in_v, n, n_vec, a_out_v, s_out_v, report))
    return MSM_AMD_INPUT_ERROR;
  report[0] = report[1] = report[2] = report[3] = 0;
  const size_t total = n * n_vec;
  if (total == 0) return MSM_AMD_OK;
  std::vector<uint8_t> sorted;
  if (arrangement == kPermuteHalo2) {
    sorted.resize(n_rows * 32);
    if (int rc = host_fr_sort(layout, table_v, n_rows, 1, threads, sorted.data(), nullptr)) return rc;
    table_v = sorted.data();
  }
  const uint8_t *table = (const uint8_t*)table_v, *in = (const uint8_t*)in_v;
  uint8_t *a_out = (uint8_t*)a_out_v, *s_out = (uint8_t*)s_out_v;
  HostIndex index;
  if (!index.build(layout, table, n_rows, threads)) return MSM_AMD_PIPELINE_ERROR;
  std::vector<uint32_t> counters(n_rows * n_vec, 0);
  const unsigned T = worker_count(threads, total);
  std::vector<uint64_t> missing(T, 0), first(T, ~(uint64_t)0);
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    HostMem probe{index.rows.data(), index.slots.data()};
    for (size_t i = lo; i < hi; ++i) {
      bool exhausted;
      const uint32_t idx = fr_lookup_find(index.plan, probe, host_get(layout, in, i), &exhausted);
      if (idx == kLookupEmpty) {
        if (!missing[t]++) first[t] = i;
      } else {
        __atomic_fetch_add(&counters[(i / n) * n_rows + idx], 1u, __ATOMIC_RELAXED);
      }
    }
  });
  report[1] = ~(uint64_t)0;
  for (unsigned t = 0; t < T; ++t) report[0] += missing[t], report[1] = std::min(report[1], first[t]);
  for (uint32_t c : counters) report[2] += c != 0, report[3] = std::max<uint64_t>(report[3], c);
  if (report[0]) return MSM_AMD_INPUT_ERROR;
  const FrPermutePlan plan = fr_permute_plan(n_rows, n_vec, kPermuteTileLog);
  std::vector<uint64_t> pairs(n_rows);
  std::vector<uint32_t> unused(n_rows);
  for (size_t v = 0; v < n_vec; ++v) {
    const uint32_t* c = counters.data() + v * n_rows;
    uint64_t run = 0;
    for (size_t j = 0; j < n_rows; ++j) {
      pairs[j] = run;
      if (c[j] == 0) unused[fr_permute_ub(run)] = (uint32_t)j;
      run += fr_permute_pair(c[j]);
    }
    const uint32_t gaps = fr_permute_unused_rows(pairs[n_rows - 1], c[n_rows - 1]);
    for_ranges(worker_count(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
      for (size_t p = lo; p < hi; ++p) {
        const uint32_t j = fr_permute_owner(pairs.data(), (uint32_t)n_rows, plan.search_steps, (uint32_t)p);
        if (a_out) host_put(layout, a_out, v * n + p, index.rows[j]);
        if (!s_out) continue;
        uint32_t k = 0;
        const bool head = fr_permute_head((uint32_t)p, j, pairs[j], &k);
        host_put(layout, s_out, v * n + p, index.rows[head ? j : unused[fr_permute_gap(arrangement, k, gaps)]]);
      }
    });
  }
  return MSM_AMD_OK;
}

}  // namespace msm_amd

extern "C" {

int msm_amd_host_fr_lookup_permute(int scalar_layout, const void* table, size_t n_rows, const void* in, size_t n, size_t n_vec,
                                   int threads, void* a_out, void* s_out, uint64_t report[4]) {
  return msm_amd::host_fr_lookup_permute(scalar_layout, msm_amd::kPermuteRows, table, n_rows, in, n, n_vec, threads, a_out, s_out,
                                         report);
}

int msm_amd_host_fr_lookup_permute_as(int scalar_layout, int arrangement, const void* table, size_t n_rows, const void* in,
                                      size_t n, size_t n_vec, int threads, void* a_out, void* s_out, uint64_t report[4]) {
  return msm_amd::host_fr_lookup_permute(scalar_layout, arrangement, table, n_rows, in, n, n_vec, threads, a_out, s_out, report);
}

int msm_amd_test_fr_permute_plan(size_t n_rows, size_t n_vec, uint32_t tile_log, uint64_t out[4]) {
  if (n_rows == 0 || n_vec == 0 || ((uint64_t)n_rows >> 31) || ((uint64_t)n_vec >> 32) ||
      (((uint64_t)n_rows * n_vec) >> 32) || tile_log < msm_amd::kPermuteMinTileLog || tile_log > msm_amd::kPermuteTileLog || !out)
    return MSM_AMD_INPUT_ERROR;
  const msm_amd::FrPermutePlan p = msm_amd::fr_permute_plan(n_rows, n_vec, tile_log);
  out[0] = p.scan.levels, out[1] = p.launches, out[2] = p.scan.tiles[0] * n_vec, out[3] = p.bytes;
  return MSM_AMD_OK;
}

int msm_amd_host_fr_lookup_multiplicities(int scalar_layout, int on_missing, const void* table, size_t n_rows, const void* in,
                                          size_t n, size_t n_vec, int threads, void* m_out, uint32_t* idx_out,
                                          uint64_t report[4]) {
  return msm_amd::host_fr_lookup_multiplicities(scalar_layout, on_missing, table, n_rows, in, n, n_vec, threads, m_out, idx_out,
                                                report);
}

int msm_amd_test_fr_lookup_plan(size_t n_rows, uint32_t hash_bits, uint64_t out[4]) {
  if (n_rows == 0 || ((uint64_t)n_rows >> 31) || hash_bits > msm_amd::kLookupAllBits || !out) return MSM_AMD_INPUT_ERROR;
  const msm_amd::FrLookupPlan p = msm_amd::fr_lookup_plan(n_rows, hash_bits);
  out[0] = p.capacity, out[1] = p.bytes, out[2] = p.home_bits, out[3] = p.slots_off;
  return MSM_AMD_OK;
}

}  // extern "C"
