// Sparse matrix times vector over BN254 Fr (msm_amd_fr_matrix_*, msm_amd_fr_matvec*): the plan and the device image of a
// matrix, shared by the host driver (msm_host.hip), the host side of the build (host_fr.hip), the kernels (k_fr.hip) and
// the test tap.  Host code only: nothing here runs on the device.
//
// A matrix is CSR: y[i] = sum_{k in [row_ptr[i], row_ptr[i+1])} values[k] x[col_idx[k]].  Rows are of very unequal length
// (an R1CS has a mean near 3, a few rows of a thousand entries and the odd one of n / 4), so the rows are cut into two
// classes by a pure planner (fr_mat_plan):
//   lane path   rows of at most LONG entries: one lane per row, consecutive lanes on consecutive rows in natural order, so
//               that y is stored at unit stride; a lane whose row is of the other class stores nothing.  One wave per 64
//               consecutive rows, whatever their class.
//   wave path   longer rows, cut into segments of at most SEG = 2^seg_log entries (all full but the last): one wave per
//               segment, lane l takes the entries l, l + 64, ... of it, six xor-shuffle additions fold the lanes, lane 0
//               stores.  A row of one segment stores to y[row]; a row of several (a split row) stores raw partial sums to
//               consecutive slots of ctx-owned memory, and a fold launch behind it in stream order -- one wave per split
//               row -- sums them into y[row].
// Launches: 1 (lane) + 1 if there is a wave row + 1 if there is a split row, ordered by the stream only.
// The values are reduced and deduplicated at build: the device holds (column, dictionary id) per entry, 8 bytes, and one
// 32-byte Montgomery record per distinct value.  Ids 0 and 1 are pinned to 1 and r - 1, present or not, for the kernels that
// add and subtract such entries without a product (MSM_AMD_FR_MAT_SIGNS).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace msm_amd {

constexpr uint32_t kFrMatLong = 32;        // rows above this many entries leave the lane path (MSM_AMD_FR_MAT_LONG)
constexpr uint32_t kFrMatSegLog = 8;       // entries per wave-path segment, as a power of two (MSM_AMD_FR_MAT_SEG_LOG)
constexpr uint32_t kFrMatMinLong = 1, kFrMatMaxLong = 4096, kFrMatMinSegLog = 6, kFrMatMaxSegLog = 20;
constexpr uint32_t kFrMatDirect = 0xFFFFFFFFu;   // FrMatSeg::slot of a row of one segment: the wave stores y[row]

struct FrMatSeg {
  uint32_t row, first, count, slot;   // entries first .. first + count of the matrix; the partial slot, or kFrMatDirect
};
struct FrMatSplit {
  uint32_t row, slot, count, pad;     // the partials slot .. slot + count are the segments of `row`, in order
};
static_assert(sizeof(FrMatSeg) == 16 && sizeof(FrMatSplit) == 16, "one dwordx4 per record");

struct FrMatPlan {
  uint64_t lane_rows, wave_rows, segments, split_rows, partials;
  uint64_t launches;   // 1, 2 or 3
  uint64_t waves;      // dispatched: ceil(n_rows / 64) of the lane path, one per segment, one per split row
};

// row_ptr: n_rows + 1 non-decreasing offsets from 0, below 2^32; long_rows and seg_log inside their ranges.  segs / splits
// (optional) receive every record.
inline FrMatPlan fr_mat_plan(uint64_t n_rows, const uint64_t* row_ptr, uint32_t long_rows, uint32_t seg_log,
                             std::vector<FrMatSeg>* segs, std::vector<FrMatSplit>* splits) {
  FrMatPlan p{};
  const uint64_t seg = (uint64_t)1 << seg_log;
  for (uint64_t i = 0; i < n_rows; ++i) {
    const uint64_t first = row_ptr[i], len = row_ptr[i + 1] - first;
    if (len <= long_rows) {
      ++p.lane_rows;
      continue;
    }
    ++p.wave_rows;
    const uint64_t pieces = (len + seg - 1) >> seg_log;
    if (pieces > 1) {
      if (splits) splits->push_back(FrMatSplit{(uint32_t)i, (uint32_t)p.partials, (uint32_t)pieces, 0u});
      ++p.split_rows;
    }
    for (uint64_t s = 0; s < pieces; ++s) {
      const uint64_t at = s << seg_log, cnt = len - at < seg ? len - at : seg;
      const uint32_t slot = pieces > 1 ? (uint32_t)(p.partials + s) : kFrMatDirect;
      if (segs) segs->push_back(FrMatSeg{(uint32_t)i, (uint32_t)(first + at), (uint32_t)cnt, slot});
    }
    p.segments += pieces;
    if (pieces > 1) p.partials += pieces;
  }
  p.launches = 1 + (p.wave_rows ? 1 : 0) + (p.split_rows ? 1 : 0);
  p.waves = (n_rows + 63) / 64 + p.segments + p.split_rows;
  return p;
}

// The one device allocation of a matrix: every part starts at a multiple of 32 bytes.
struct FrMatImage {
  size_t row_off;   // n_rows + 1 u32
  size_t ent;       // nnz (column, dictionary id) pairs of u32
  size_t dict;      // the dictionary: 1, r - 1, then every other distinct value; reduced Montgomery residues
  size_t segs;      // FrMatSeg
  size_t splits;    // FrMatSplit
  size_t bytes;     // >= 32
};
inline FrMatImage fr_mat_image(uint64_t n_rows, uint64_t nnz, uint64_t dict_records, const FrMatPlan& p) {
  auto up = [](size_t b) { return (b + 31) & ~(size_t)31; };
  FrMatImage m{};
  m.row_off = 0;
  m.ent = up((n_rows + 1) * 4);
  m.dict = m.ent + up(nnz * 8);
  m.segs = m.dict + up(dict_records * 32);
  m.splits = m.segs + up(p.segments * sizeof(FrMatSeg));
  m.bytes = m.splits + up(p.split_rows * sizeof(FrMatSplit));
  if (m.bytes < 32) m.bytes = 32;
  return m;
}

}  // namespace msm_amd
