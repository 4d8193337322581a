// Launch wrappers of the Fr vector kernels (k_fr.hip) for the host driver (msm_host.hip), and the argument checks the
// driver shares with the host twin (host_fr.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fr_vec.hip.h"

namespace msm_amd {

// out[i] = op(k, a[i], b[i], c[i]), i < n; k Montgomery and reduced; operands the op does not read may be null
void launch_fr_map(hipStream_t st, int op, int layout, const u256& k, const void* a, const void* b, const void* c, size_t n,
                   void* out);

struct FrScanLaunch {
  const void* in;     // n_vec * n records; in == out is allowed
  void* out;
  void* work;         // fr_scan_plan(n, n_vec, tile_log).records records (may be null for a plan of one level)
  uint64_t n, n_vec;
  uint32_t tile_log;
  int layout;         // of in and out: a scalar layout, or kFrRaw
  int mode;           // kFrInclusive, kFrExclusive
  bool reverse;       // the suffix products: every vector is scanned from its last record down
};
// every launch of one scan, in stream order; returns the number of launches
uint32_t launch_fr_scan(hipStream_t st, const FrScanLaunch& c);

// The first span of an inversion: the tile products of `in` with zeros read as one, their inclusive prefix (P) and
// suffix (S) products in `work` (fr_inv_plan), and the number of zeros in the first 8 bytes of the record behind P.
// T and the count are the 64 bytes at fr_inv_tail(work, plan).
uint32_t launch_fr_inv_products(hipStream_t st, int layout, const void* in, uint64_t n, uint32_t tile_log, void* work);
inline const void* fr_inv_tail(const void* work, const FrInvPlan& p) {
  return (const uint8_t*)work + (p.p_off + p.tiles - 1) * 32;
}
// The second span: out[i] = in[i]^-1 (0 for 0) from P, S and t_inv = T^-1 (Montgomery)
void launch_fr_inv_apply(hipStream_t st, int layout, const void* in, uint64_t n, uint32_t tile_log, const void* work,
                         const u256& t_inv, void* out);

// host_fr.hip.  Each check returns null or what is wrong, for msm_amd_last_error.
bool fr_layout_known(int scalar_layout);   // MONT_LE and CANON_LE
bool fr_mode_known(int mode);
// the k of a call -> reduced Montgomery residue (one for an op without k)
u256 fr_read_k(int op, int scalar_layout, const void* k32);
// `bytes` at out against the same number at p: equal or disjoint
bool fr_overlap_ok(const void* out, const void* p, size_t bytes);
const char* fr_map_check(int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c, size_t n,
                         const void* out, bool device);
const char* fr_unary_check(int scalar_layout, const void* in, uint64_t n, uint64_t n_vec, const void* out, bool device);

}  // namespace msm_amd
