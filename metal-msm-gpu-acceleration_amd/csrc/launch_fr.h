// Launch wrappers of the Fr vector kernels (k_fr.hip; the lookup tables: k_lookup.hip, k_permute.hip) for the host driver
// (calls_fr.hip), and the argument checks the driver shares with the host twins (host_fr.hip, host_lookup.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fr_gate.hip.h"
#include "fr_lookup.hip.h"
#include "fr_permute.hip.h"
#include "fr_mat.hip.h"
#include "fr_mle.hip.h"
#include "fr_poseidon.hip.h"
#include "fr_sort.hip.h"
#include "fr_vec.hip.h"

struct msm_amd_fr_sumcheck_terms;   // include/msm_amd.h
struct msm_amd_fr_gate_terms;

namespace msm_amd {

// out[i] = op(k, a[i], b[i], c[i]), i < n; k Montgomery and reduced; operands the op does not read may be null
void launch_fr_map(hipStream_t st, int op, int layout, const u256& k, const void* a, const void* b, const void* c, size_t n,
                   void* out);
// out[i] = a[i] + k, i < n; one more instantiation of the map kernel
void launch_fr_shift(hipStream_t st, int layout, const u256& k, const void* a, size_t n, void* out);

struct FrScanLaunch {
  const void* in;     // n_vec * n records; in == out is allowed
  void* out;
  void* work;         // fr_scan_plan(n, n_vec, tile_log).records records (may be null for a plan of one level)
  uint64_t n, n_vec;
  uint32_t tile_log;
  int layout;         // of in and out: a scalar layout, or kFrRaw
  int mode;           // kFrInclusive, kFrExclusive
  bool reverse;       // the suffix products: every vector is scanned from its last record down
  bool sum;           // the running sums (msm_amd_fr_prefix_sum*): the same plan over addition, an exclusive scan starts at 0
};
// every launch of one scan, in stream order; returns the number of launches
uint32_t launch_fr_scan(hipStream_t st, const FrScanLaunch& c);

// Polynomials over Fr: n_vec vectors of n coefficients, lowest degree first, on the tiles and levels of fr_scan_plan.
// Level k + 1 holds the values H_b = sum_m c_(b 2^T + m) x^m of the tiles of level k at that level's point x =
// z^(2^(T k)): the same problem at the point x^(2^T).  Tiles start at index 0 of a vector, so every tile that has a
// successor is full and every multiplier is uniform.
//   evaluation  levels reductions, the last one leaves p_v(z)
//   division    levels - 1 reductions, then the scan s_i = sum_(j >= i) c_j x^(j - i) of every level from the top down,
//               every tile starting from s of the level above; level 0 writes out[i] = s_(i+1), out[n - 1] = 0, and
//               the top level leaves s_0 = p_v(z)
// The n_vec values p_v(z) are raw records (reduced Montgomery residues) behind the totals: work + fr_poly_values(plan).
// z^(2^j), j < 48: level k reads j from T k up to T k + max(6, T - 1), and T k < 32 because 2^(T k) < n < 2^32
constexpr uint32_t kFrPolyPowers = 48;
struct FrPolyLaunch {
  const void* in;     // n_vec * n records
  void* out;          // division: n_vec * n records, in == out is allowed
  void* work;         // fr_scan_plan(n, n_vec, tile_log).records + n_vec records
  uint64_t n, n_vec;
  uint32_t tile_log;
  int layout;
  bool divide;
  u256 z;             // Montgomery and reduced
};
inline size_t fr_poly_values(const FrScanPlan& p) { return (size_t)p.records * 32; }
// every launch of one evaluation or division, in stream order; returns the number of launches
uint32_t launch_fr_poly(hipStream_t st, const FrPolyLaunch& c);
// The same at k points in one pass (fr_vec.hip.h): evaluation leaves p_v(z_j), division the quotient by prod_j (X - z_j)
// and p_v(z_j).  The levels >= 1 of the plan exist once per point: point j owns the records j plan.records .. of the
// workspace, and the k n_vec values lie behind all of them, point-major (value of point j, vector v at j n_vec + v).
// The launches are those of one point: levels for an evaluation, 2 levels - 1 for a division.
struct FrPolyPointsLaunch {
  const void* in;     // n_vec * n records
  void* out;          // division: n_vec * n records, in == out is allowed
  void* work;         // fr_poly_points_records(plan, n_vec, k) records
  uint64_t n, n_vec;
  uint32_t tile_log;
  int layout;
  bool divide;
  uint32_t k;                    // 1 .. kFrPolyMaxPoints
  u256 z[kFrPolyMaxPoints];      // Montgomery and reduced; a division: pairwise distinct
};
inline size_t fr_poly_points_values(const FrScanPlan& p, uint64_t k) { return (size_t)(k * p.records) * 32; }
inline uint64_t fr_poly_points_records(const FrScanPlan& p, uint64_t n_vec, uint64_t k) { return k * (p.records + n_vec); }
uint32_t launch_fr_poly_points(hipStream_t st, const FrPolyPointsLaunch& c);
// out[i] = sum_v k^v a[v n + i], i < n; out may be a
void launch_fr_lincomb(hipStream_t st, int layout, const u256& k, const void* a, uint64_t n, uint64_t n_vec, void* out);

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

// y = M x (fr_mat.hip.h): the lane launch, the wave launch if the plan has a wave row, the fold launch if it has a
// split row, in stream order; returns the number of launches
struct FrMatLaunch {
  const void* image;   // the device allocation of the matrix (FrMatImage)
  FrMatImage at;
  FrMatPlan plan;
  uint64_t n_rows;
  uint32_t long_rows;
  int layout;          // of x and y
  bool signs;          // the kernels that add and subtract entries of value 1 and r - 1 without a product
  const void* x;       // n_cols records
  void* y;             // n_rows records, disjoint from x
  void* work;          // plan.partials raw records (may be null without a split row)
};
uint32_t launch_fr_matvec(hipStream_t st, const FrMatLaunch& c);

// Multilinear tables and sumcheck rounds (fr_mle.hip.h).  Tables lie `stride` records apart; challenges are reduced
// Montgomery residues in the order of LOW: r[j] meets variable x_j (the driver reverses the point of a HIGH evaluation).
struct FrMleRoundLaunch {
  const void* in;      // n_vec tables of n records
  void* work;          // fr_mle_round_plan(n, d + 1, chunk_log).records raw records; the d + 1 values at values_off
  uint64_t n, n_vec, stride;
  uint32_t chunk_log;
  int layout, order, form;
};
uint32_t launch_fr_sumcheck_round(hipStream_t st, const FrMleRoundLaunch& c);
// A round over a term list; step: a bind launch of every table at r into `out` first, the sums over the n / 2 records left
struct FrTermRoundLaunch {
  const void* in;      // n_vec tables of n records
  void* out;           // step: the bound tables (HIGH: may be in)
  void* work;          // fr_mle_round_plan(step ? n / 2 : n, d + 1, chunk_log).records raw records
  uint64_t n, n_vec, stride;
  uint32_t chunk_log;
  int layout, order;
  bool step;
  u256 r;
  FrSumTerms terms;
};
uint32_t launch_fr_sumcheck_terms(hipStream_t st, const FrTermRoundLaunch& c);
// A gate polynomial over rotated columns (fr_gate.hip.h): one launch, one lane per row
struct FrGateLaunch {
  const void* in;      // n_vec columns of n records, `stride` records apart
  const void* acc;     // accumulate: the n records out[i] is computed from (out itself, or a staged copy of it)
  const void* scale;   // optional: `period` raw records (reduced Montgomery residues)
  void* out;           // n records, disjoint from in
  uint64_t n, stride;
  uint32_t period;     // a power of two that divides n
  int layout;
  bool accumulate;
  u256 k_acc;          // Montgomery and reduced
  FrGateTerms terms;
};
void launch_fr_gate(hipStream_t st, const FrGateLaunch& c);
struct FrMleEvalLaunch {
  const void* in;
  void* work;          // fr_scan_plan(n, n_vec, tile_log).records + n_vec raw records; the n_vec values behind the levels
  uint64_t n, n_vec, stride;
  uint32_t tile_log;
  int layout;
  u256 r[kFrMleMaxVars];   // r[j] meets x_j
};
uint32_t launch_fr_mle_eval(hipStream_t st, const FrMleEvalLaunch& c);
struct FrMleBindLaunch {
  const void* in;
  void* out;           // HIGH: may be in
  void* work;          // fr_mle_bind_plan(..).work_records raw records (may be null for none)
  uint64_t n, n_vec, stride;
  uint32_t n_bind;
  int layout, order;
  u256 r[kFrMleMaxVars];   // r[s] is the challenge of step s of `order`
};
uint32_t launch_fr_mle_bind(hipStream_t st, const FrMleBindLaunch& c);
// out[i] = prod_b (bit b of i ? point_by_bit[b] : 1 - point_by_bit[b]), i < 2^m
void launch_fr_eq_table(hipStream_t st, int layout, const u256* point_by_bit, uint32_t m, void* out);

// Poseidon (fr_poseidon.hip.h).  `image` is the constants image of a parameter handle in device memory; the tag is a reduced
// Montgomery residue.  Every pointer is 16-byte aligned device memory.
struct PoseidonLaunch {
  const void* image;
  uint32_t t, r_f, r_p;
  int layout;
  u256 tag;            // hash and tree
};
// n states of t records -> n states (kPoseidonPermute, out may be in), or n groups of t - 1 records -> n digests
// (kPoseidonHash; out is in only for t = 2, else disjoint from it: see fr_poseidon_kernel)
void launch_poseidon(hipStream_t st, const PoseidonLaunch& c, int kind, const void* in, uint64_t n, void* out);
// every launch of poseidon_tree_plan(n_leaves, t - 1, top_log) in stream order; returns the number of launches
uint32_t launch_poseidon_tree(hipStream_t st, const PoseidonLaunch& c, const void* leaves, uint64_t n_leaves, uint32_t top_log,
                              void* tree);
// out: depth (arity - 1) sibling records per index, bottom level first; idx: n_idx checked leaf indices in device memory
void launch_merkle_paths(hipStream_t st, int layout, uint32_t arity, uint32_t depth, const void* leaves, uint64_t n_leaves,
                         const void* tree, const void* idx, uint64_t n_idx, void* out);

// Lookup tables (fr_lookup.hip.h).  The build fills the slots and the statistics of an image whose rows are there already
// (d_table null: uploaded as residues) or come from d_table, n_rows records of `layout` in device memory.
void launch_fr_lookup_build(hipStream_t st, const FrLookupPlan& plan, uint64_t n_rows, int layout, const void* d_table,
                            void* image);
struct FrLookupLaunch {
  const void* image;   // the device allocation of the handle
  FrLookupPlan plan;
  uint64_t n_rows;
  int layout, on_missing, count_form;
  const void* in;      // total records
  uint64_t total;      // n * n_vec; may be 0
  void* m_out;         // n_rows records
  uint32_t* idx_out;   // optional: total words
  void* work;          // fr_lookup_work: counters and report, cleared by the launch
  FrLookupWork at;
};
// the clears, the probe launch (if there are inputs) and the finish launch, in stream order; returns the number of kernels
uint32_t launch_fr_lookup_multiplicities(hipStream_t st, const FrLookupLaunch& c);
// the probe launch alone (total >= 1), into cleared counters and a cleared report.  col_n == 0: n_rows counters; else input i
// belongs to column i / col_n and counts in counters[(i / col_n) n_rows + row]
void launch_fr_lookup_probe(hipStream_t st, const FrLookupLaunch& c, uint64_t col_n, uint32_t* counters,
                            unsigned long long* report);

// halo2's permuted columns (fr_permute.hip.h, k_permute.hip): the clears, the probe, the scan with the compaction, the fill,
// in stream order; returns the number of kernels.  n >= 1, n_vec >= 1.
struct FrPermuteLaunch {
  FrLookupLaunch probe;   // image, plan, n_rows, layout, count_form, in, total = n n_vec; m_out, idx_out, work, at unused
  FrPermutePlan plan;
  uint32_t tile_log;
  int fill_form;          // kPermuteFillSearch, kPermuteFillScan
  int arrangement;        // kPermuteRows, kPermuteHalo2 (the handle is sorted)
  uint64_t n, n_vec;
  void* a_out;            // optional: total records; may be probe.in
  void* s_out;            // optional: total records, n == n_rows
  void* work;             // plan.bytes; kPermuteFillScan: fr_permute_owner_plan(plan, n, n_vec, tile_log).bytes
};
uint32_t launch_fr_lookup_permute(hipStream_t st, const FrPermuteLaunch& c);

// The sort by canonical value (fr_sort.hip.h, k_fr_sort.hip) in its two spans: the keys with the digit mask, left in the
// first word of the 64-byte record at the start of the workspace, and, once the host has read the mask, the passes and the
// final gather of every column; the second returns its number of kernels.  n >= 1, n_vec >= 1, n n_vec < 2^32.
struct FrSortLaunch {
  const void* in;         // n n_vec records; read by the first span only, so out may be in
  void* out;              // optional: n n_vec records
  uint32_t* perm_out;     // optional: n n_vec words, column-relative
  void* work;             // plan.bytes
  FrSortPlan plan;        // of any mask: the workspace does not depend on it
  uint64_t n, n_vec;
  int layout;
};
void launch_fr_sort_keys(hipStream_t st, const FrSortLaunch& c);
uint32_t launch_fr_sort_passes(hipStream_t st, const FrSortLaunch& c, uint32_t mask);

// host_fr.hip.  Each check returns null or what is wrong, for msm_amd_last_error.
bool fr_layout_known(int scalar_layout);   // MONT_LE and CANON_LE
bool fr_mode_known(int mode);
// the k of a call -> reduced Montgomery residue (one for an op without k)
u256 fr_read_k(int op, int scalar_layout, const void* k32);
// `bytes` at out against the same number at p: equal or disjoint
bool fr_overlap_ok(const void* out, const void* p, size_t bytes);
const char* fr_map_check(int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c, size_t n,
                         const void* out, bool device);
// one record in host memory -> reduced Montgomery residue
u256 fr_read_record(int scalar_layout, const void* rec32);
// msm_amd_fr_poly_eval* (values required, out unused) and msm_amd_fr_poly_div_linear* (out required, values optional)
const char* fr_poly_check(int scalar_layout, const void* z32, const void* in, uint64_t n, uint64_t n_vec, const void* out,
                          const void* values, bool divide, bool device);
// msm_amd_fr_poly_eval_points (values required, out unused), msm_amd_fr_poly_div_points (out required, values optional)
// and their twins (mem: MSM_AMD_MEM_HOST): layout, mem, k and z first, then the sizes, then n == 0 or n_vec == 0 passes,
// then pointers, alignment (device), overlap and, for a division, that no two points are equal mod r.  The message of that
// last refusal names both indices and lives in a buffer of the calling thread.
const char* fr_poly_points_check(int mem, int scalar_layout, const void* z, uint64_t k, const void* in, uint64_t n,
                                 uint64_t n_vec, const void* out, const void* values, bool divide);
// w_j = 1 / prod_(m != j) (z_j - z_m) of pairwise distinct reduced residues, one inversion for all (k == 1: one)
void fr_poly_points_weights(const u256* z, uint32_t k, u256* w);
// msm_amd_fr_lincomb*: out is the first vector of a or disjoint from all of a
const char* fr_lincomb_check(int scalar_layout, const void* k32, const void* a, uint64_t n, uint64_t n_vec, const void* out,
                             bool device);
const char* fr_unary_check(int scalar_layout, const void* in, uint64_t n, uint64_t n_vec, const void* out, bool device);
// msm_amd_fr_shift*: out is a itself or disjoint from it
const char* fr_shift_check(int scalar_layout, const void* k32, const void* a, uint64_t n, const void* out, bool device);
// host_lookup.hip.  A table: 1 <= n_rows < 2^31
const char* fr_lookup_table_check(int scalar_layout, const void* table, uint64_t n_rows, bool device);
// msm_amd_fr_lookup_multiplicities*: layout and mode first, then the sizes; n == 0 or n_vec == 0 needs m_out only
const char* fr_lookup_call_check(int scalar_layout, int on_missing, uint64_t n_rows, const void* in, uint64_t n, uint64_t n_vec,
                                 const void* m_out, const uint32_t* idx_out, const uint64_t* report, bool device);
// MSM_AMD_LOOKUP_HASH_BITS (0 .. 32, default all) and MSM_AMD_LOOKUP_COUNT (lane / wave), read at every call
uint32_t fr_lookup_hash_bits_knob();
int fr_lookup_count_knob();
// msm_amd_fr_lookup_permute and its twin: layout, report and the outputs first, then n == 0 or n_vec == 0 passes, then sizes, pointers
// and overlap: a_out may be `in` itself, every other pair of in, a_out, s_out is disjoint
const char* fr_permute_call_check(int scalar_layout, uint64_t n_rows, const void* in, uint64_t n, uint64_t n_vec,
                                  const void* a_out, const void* s_out, const uint64_t* report);
// MSM_AMD_PERMUTE_TILE_LOG (2 .. kPermuteTileLog, the default), read at every call
uint32_t fr_permute_tile_log_knob();
// MSM_AMD_PERMUTE_FILL (search / scan), read at every call
int fr_permute_fill_knob();
// host_fr_sort.hip.  msm_amd_fr_sort and its twin: mem and layout first, then the outputs, then n == 0 or n_vec == 0 passes,
// then sizes, pointers, alignment (device) and overlap: out may be `in` itself, every other pair of in, out, perm_out is disjoint
const char* fr_sort_call_check(int mem, int scalar_layout, const void* in, uint64_t n, uint64_t n_vec, const void* out,
                               const uint32_t* perm_out);
// the twin of the sort itself, for the twin of the permuted columns in value order (host_lookup.hip)
int host_fr_sort(int layout, const void* in, size_t n, size_t n_vec, int threads, void* out, uint32_t* perm_out);
// a CSR matrix in host memory (msm_amd_fr_matrix_build, msm_amd_host_fr_matvec): sizes, row_ptr and EVERY column
const char* fr_matrix_check(int scalar_layout, uint64_t n_rows, uint64_t n_cols, const uint64_t* row_ptr,
                            const uint32_t* col_idx, const void* values);
// x (n_cols records) and y (n_rows records) of a product: out of place only, no overlap of any kind
const char* fr_matvec_check(int scalar_layout, uint64_t n_rows, uint64_t n_cols, const void* x, const void* y, bool device);
// The multilinear calls.  Every check first looks at layout, order and form, then lets n_vec == 0 pass (nothing to do), then
// at the sizes, the pointers and the overlap rules.  fr_mle_tables_check is the part they share: n a power of two, 2 <= n <
// 2^32, stride >= n, n_vec stride < 2^32.
const char* fr_mle_tables_check(uint64_t n, uint64_t n_vec, uint64_t stride);
const char* fr_mle_bind_check(int scalar_layout, int order, const void* r, uint64_t n_bind, const void* in, uint64_t n,
                              uint64_t n_vec, uint64_t stride, const void* out, bool device);
const char* fr_mle_eval_check(int scalar_layout, int order, const void* point, const void* in, uint64_t n, uint64_t n_vec,
                              uint64_t stride, const void* y_out, bool device);
const char* fr_eq_table_check(int scalar_layout, int order, const void* point, uint64_t m, const void* out, bool device);
const char* fr_sumcheck_check(int scalar_layout, int order, int form, const void* in, uint64_t n, uint64_t n_vec,
                              uint64_t stride, const void* g_out, bool device);
// The term list of msm_amd_fr_sumcheck_round_terms* / _step_terms*: its sizes, pointers and indices (no ctx); on success
// and with `image` given, the image the kernels and the twins run on.  fr_sumcheck_terms_round_check and
// fr_sumcheck_step_check are the whole checks of the two calls; n_vec == 0 passes them before the list is looked at.
const char* fr_sumcheck_terms_check(int scalar_layout, const ::msm_amd_fr_sumcheck_terms* terms, uint64_t n_vec,
                                    FrSumTerms* image);
const char* fr_sumcheck_terms_round_check(int scalar_layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* in,
                                          uint64_t n, uint64_t n_vec, uint64_t stride, const void* g_out, bool device,
                                          FrSumTerms* image);
const char* fr_sumcheck_step_check(int scalar_layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* r,
                                   const void* in, uint64_t n, uint64_t n_vec, uint64_t stride, const void* out,
                                   const void* g_out, bool device, FrSumTerms* image);
// The term list of msm_amd_fr_gate_eval and its twin against n_vec columns of n rows (msm_amd_fr_gate_check; no ctx): sizes,
// pointers, indices, rot_step and the number of distinct offsets (rot rot_step) mod n; on success and with `image` given,
// the image the kernel and the twin run on; its coefficients are read (in scalar_layout) only with `coeffs`.
const char* fr_gate_terms_check(int scalar_layout, const ::msm_amd_fr_gate_terms* terms, uint64_t n_vec, uint64_t n,
                                uint64_t rot_step, FrGateTerms* image, bool coeffs);
// The whole check of the call: layout, mem and flags first, then n >= 2^32, then n == 0 or n_vec == 0 passes, then the list,
// the stride, the pointers the call reads, the period of a scale, alignment (device) and the overlap of out and in
const char* fr_gate_eval_check(int mem, int scalar_layout, uint32_t flags, const ::msm_amd_fr_gate_terms* terms, const void* in,
                               uint64_t n, uint64_t n_vec, uint64_t stride, uint64_t rot_step, const void* k_acc32,
                               const void* scale, uint64_t period, const void* out, FrGateTerms* image);
// The Poseidon calls.  The shape (t, r_f, r_p) is that of a parameter handle or of the twin's arguments; every check first
// looks at the layout, then at the sizes, lets n == 0 pass where a call has one, then at pointers, alignment and overlap.
const char* poseidon_shape_check(uint64_t t, uint64_t r_f, uint64_t r_p);
const char* poseidon_constants_check(uint64_t t, uint64_t r_f, uint64_t r_p, int scalar_layout, const void* ark, const void* mds);
// kind: kPoseidonPermute (n t records in and out, out == in or disjoint) or kPoseidonHash (n (t - 1) in, n out)
const char* poseidon_call_check(int kind, uint32_t t, int scalar_layout, const void* in, uint64_t n, const void* out, bool device);
const char* poseidon_merkle_check(uint32_t t, int scalar_layout, const void* leaves, uint64_t n_leaves, const void* tree,
                                  bool device);
// idx in host memory: every index is looked at
const char* poseidon_paths_check(uint32_t t, int scalar_layout, const void* leaves, uint64_t n_leaves, const void* tree,
                                 const uint64_t* idx, uint64_t n_idx, const void* out, bool device);
// the constants of a caller in host memory -> the image of poseidon_image_records(t, r_f + r_p) reduced Montgomery residues
void poseidon_build_image(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                          std::vector<u256>* image);
// The device image of a checked matrix in host memory: values reduced mod r and deduplicated into the dictionary (ids 0
// and 1 are always 1 and r - 1, whether they occur or not: dict_records counts them, n_distinct only what occurs), the
// plan at (long_rows, seg_log), every part at its place of fr_mat_image
void fr_mat_build_image(int scalar_layout, uint64_t n_rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                        const void* values, uint32_t long_rows, uint32_t seg_log, FrMatPlan* plan, FrMatImage* at,
                        uint64_t* n_distinct, uint64_t* dict_records, std::vector<uint8_t>* image);

}  // namespace msm_amd
