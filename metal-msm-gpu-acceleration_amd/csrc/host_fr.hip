// Host twins of the Fr vector calls (no ctx, no GPU): the load, store and op bodies of fr_vec.hip.h on the CPU, the
// records split over the host threads -- the map record by record, the inversion with one inversion per range (the
// classic trick), the prefix products in two phases (the product of every range, then the ranges from their carries),
// the polynomial calls likewise (a range's Horner value, then the ranges from the sums behind them; at several points: k
// evaluations and k chained divisions, upstream's div_by_vanishing), the sparse product
// row by row over ranges of equal entry count, the multilinear calls step by step over ranges of outputs (a round: the sums
// of every range of pairs, added in range order), the Poseidon calls permutation by permutation over ranges, a tree level by
// level, a round over a term list as the sums of every range of pairs in range order and its step as the bind followed by
// that round, a gate polynomial over rotated columns row by row over ranges of rows (and the constants of the paper's Grain
// generator, msm_amd_poseidon_constants);
// and the argument checks the twins share with the host driver (msm_host.hip).  The bytes of a result are unique, so the
// way a twin cuts the work shows nowhere.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_fr.h"
#include "launch_ntt.h"

namespace msm_amd {

static_assert(kFrAdd == MSM_AMD_FR_ADD && kFrSub == MSM_AMD_FR_SUB && kFrMul == MSM_AMD_FR_MUL &&
              kFrScale == MSM_AMD_FR_SCALE && kFrAxpy == MSM_AMD_FR_AXPY && kFrMulsubScale == MSM_AMD_FR_MULSUB_SCALE, "ops");
static_assert(kFrMleLow == MSM_AMD_MLE_LOW && kFrMleHigh == MSM_AMD_MLE_HIGH && kFrSumProduct == MSM_AMD_SUMCHECK_PRODUCT &&
              kFrSumEqAbC == MSM_AMD_SUMCHECK_EQ_AB_C, "orders and forms");
static_assert(kFrInclusive == MSM_AMD_FR_PREFIX_INCLUSIVE && kFrExclusive == MSM_AMD_FR_PREFIX_EXCLUSIVE, "modes");

bool fr_layout_known(int scalar_layout) { return ntt_layout_known(scalar_layout); }
bool fr_mode_known(int mode) { return mode == kFrInclusive || mode == kFrExclusive; }

u256 fr_read_k(int op, int scalar_layout, const void* k32) {
  if (!(fr_op_reads(op) & kFrReadsK) || !k32) return Fr::one();
  uint32_t rec[8];
  std::memcpy(rec, k32, 32);
  return ntt_load(scalar_layout, rec);
}

bool fr_overlap_ok(const void* out, const void* p, size_t bytes) {
  const uintptr_t a = (uintptr_t)out, b = (uintptr_t)p;
  return a == b || a + bytes <= b || b + bytes <= a;
}

const char* fr_map_check(int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c, size_t n,
                         const void* out, bool device) {
  const unsigned reads = fr_op_reads(op);
  if (!reads) return "op must be one of MSM_AMD_FR_ADD .. MSM_AMD_FR_MULSUB_SCALE";
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if ((uint64_t)n >> 32) return "n >= 2^32";
  if (n == 0) return nullptr;
  const void* operand[3] = {a, b, c};
  if (!out || ((reads & kFrReadsK) && !k32)) return "null pointer with n > 0";
  for (int i = 0; i < 3; ++i) {
    if (!(reads & (1u << i))) continue;
    if (!operand[i]) return "null pointer for an operand the op reads";
    if (device && ((uintptr_t)operand[i] & 15u)) return "device buffers must be 16-byte aligned";
    if (!fr_overlap_ok(out, operand[i], n * 32)) return "the output must be an operand itself or disjoint from it";
  }
  if (device && ((uintptr_t)out & 15u)) return "device buffers must be 16-byte aligned";
  return nullptr;
}

const char* fr_unary_check(int scalar_layout, const void* in, uint64_t n, uint64_t n_vec, const void* out, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (n == 0 || n_vec == 0) return nullptr;
  if (!in || !out) return "null pointer with n > 0";
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return "device buffers must be 16-byte aligned";
  if (!fr_overlap_ok(out, in, n * n_vec * 32)) return "the output must be the input itself or disjoint from it";
  return nullptr;
}

const char* fr_shift_check(int scalar_layout, const void* k32, const void* a, uint64_t n, const void* out, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (n >> 32) return "n >= 2^32";
  if (n == 0) return nullptr;
  if (!k32 || !a || !out) return "null pointer with n > 0";
  if (device && (((uintptr_t)a | (uintptr_t)out) & 15u)) return "device buffers must be 16-byte aligned";
  if (!fr_overlap_ok(out, a, n * 32)) return "the output must be the input itself or disjoint from it";
  return nullptr;
}

u256 fr_read_record(int scalar_layout, const void* rec32) {
  uint32_t rec[8];
  std::memcpy(rec, rec32, 32);
  return ntt_load(scalar_layout, rec);
}

const char* fr_poly_check(int scalar_layout, const void* z32, const void* in, uint64_t n, uint64_t n_vec, const void* out,
                          const void* values, bool divide, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (n == 0 || n_vec == 0) return nullptr;
  if (!z32 || !in || (divide ? !out : !values)) return "null pointer with n > 0";
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return "device buffers must be 16-byte aligned";
  if (divide && !fr_overlap_ok(out, in, n * n_vec * 32)) return "the output must be the input itself or disjoint from it";
  return nullptr;
}

const char* fr_poly_points_check(int mem, int scalar_layout, const void* z, uint64_t k, const void* in, uint64_t n,
                                 uint64_t n_vec, const void* out, const void* values, bool divide) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE) return "mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE";
  if (k == 0 || k > kFrPolyMaxPoints) return "k must be 1 .. MSM_AMD_POLY_MAX_POINTS";
  if (!z) return "null z";
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (n == 0 || n_vec == 0) return nullptr;
  if (!in || (divide ? !out : !values)) return "null pointer with n > 0";
  if (mem == MSM_AMD_MEM_DEVICE && (((uintptr_t)in | (uintptr_t)out) & 15u)) return "device buffers must be 16-byte aligned";
  if (!divide) return nullptr;
  if (!fr_overlap_ok(out, in, n * n_vec * 32)) return "the output must be the input itself or disjoint from it";
  u256 x[kFrPolyMaxPoints];
  for (uint64_t j = 0; j < k; ++j) x[j] = fr_read_record(scalar_layout, (const uint8_t*)z + j * 32);
  for (uint64_t i = 0; i < k; ++i)
    for (uint64_t j = i + 1; j < k; ++j)
      if (u256_eq(x[i], x[j])) {
        static thread_local char why[96];
        std::snprintf(why, sizeof why, "the points %u and %u are equal mod r: the division needs distinct points", (unsigned)i,
                      (unsigned)j);
        return why;
      }
  return nullptr;
}

void fr_poly_points_weights(const u256* z, uint32_t k, u256* w) {
  // d_j = prod_(m != j) (z_j - z_m), then Montgomery's trick: one inversion of d_0 .. d_(k-1)
  u256 d[kFrPolyMaxPoints], pre[kFrPolyMaxPoints];
  u256 run = Fr::one();
  for (uint32_t j = 0; j < k; ++j) {
    d[j] = Fr::one();
    for (uint32_t m = 0; m < k; ++m)
      if (m != j) d[j] = Fr::mul(d[j], Fr::sub(z[j], z[m]));
    pre[j] = run;
    run = Fr::mul(run, d[j]);
  }
  u256 inv = ntt_fr_inv(run);   // of d_0 .. d_j
  for (uint32_t j = k; j-- != 0;) {
    w[j] = Fr::mul(inv, pre[j]);
    inv = Fr::mul(inv, d[j]);
  }
}

const char* fr_lincomb_check(int scalar_layout, const void* k32, const void* a, uint64_t n, uint64_t n_vec, const void* out,
                             bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if ((n >> 32) || (n_vec >> 32) || ((n * n_vec) >> 32)) return "n * n_vec >= 2^32";
  if (n == 0 || n_vec == 0) return nullptr;
  if (!k32 || !a || !out) return "null pointer with n > 0";
  if (device && (((uintptr_t)a | (uintptr_t)out) & 15u)) return "device buffers must be 16-byte aligned";
  const uintptr_t o = (uintptr_t)out, p = (uintptr_t)a;
  if (o != p && !(o + n * 32 <= p || p + n * n_vec * 32 <= o)) return "the output must be the first vector or disjoint from every vector";
  return nullptr;
}

const char* fr_matrix_check(int scalar_layout, uint64_t n_rows, uint64_t n_cols, const uint64_t* row_ptr,
                            const uint32_t* col_idx, const void* values) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (n_rows == 0 || n_cols == 0) return "n_rows and n_cols must be at least 1";
  if ((n_rows >> 32) || (n_cols >> 32)) return "n_rows or n_cols >= 2^32";
  if (!row_ptr) return "null row_ptr";
  if (row_ptr[0] != 0) return "row_ptr[0] must be 0";
  for (uint64_t i = 0; i < n_rows; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr must not decrease";
    if (row_ptr[i + 1] >> 32) return "nnz >= 2^32";
  }
  const uint64_t nnz = row_ptr[n_rows];
  if (nnz && (!col_idx || !values)) return "null col_idx or values with nnz > 0";
  for (uint64_t k = 0; k < nnz; ++k)
    if (col_idx[k] >= n_cols) return "a column index is not below n_cols";
  return nullptr;
}

const char* fr_matvec_check(int scalar_layout, uint64_t n_rows, uint64_t n_cols, const void* x, const void* y, bool device) {
  if (!fr_layout_known(scalar_layout)) return "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
  if (!x || !y) return "null x or y";
  if (device && (((uintptr_t)x | (uintptr_t)y) & 15u)) return "device buffers must be 16-byte aligned";
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
  if (a < b + n_rows * 32 && b < a + n_cols * 32) return "y must not overlap x: the product is out of place only";
  return nullptr;
}

namespace {
const char* const kMleLayout = "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only";
const char* const kMleOrder = "order must be MSM_AMD_MLE_LOW or MSM_AMD_MLE_HIGH";
const char* const kMleAlign = "device buffers must be 16-byte aligned";
bool spans_apart(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + a_bytes <= y || y + b_bytes <= x;
}
}  // namespace

const char* fr_mle_tables_check(uint64_t n, uint64_t n_vec, uint64_t stride) {
  if (n < 2 || (n >> 32) || (n & (n - 1))) return "n must be a power of two, 2 <= n < 2^32";
  if (stride < n) return "stride < n";
  if ((stride >> 32) || (n_vec >> 32) || ((n_vec * stride) >> 32)) return "n_vec * stride >= 2^32";
  return nullptr;
}

const char* fr_mle_bind_check(int scalar_layout, int order, const void* r, uint64_t n_bind, const void* in, uint64_t n,
                              uint64_t n_vec, uint64_t stride, const void* out, bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (n_vec == 0) return nullptr;
  if (const char* why = fr_mle_tables_check(n, n_vec, stride)) return why;
  if (n_bind == 0 || n_bind > fr_mle_log2(n)) return "n_bind must be 1 .. log2 n";
  if (!r || !in || !out) return "null pointer with work to do";
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return kMleAlign;
  if (out == in) return order == kFrMleHigh ? nullptr : "MSM_AMD_MLE_LOW is out of place only";
  if (!spans_apart(in, ((n_vec - 1) * stride + n) * 32, out, ((n_vec - 1) * stride + n / 2) * 32))
    return "the output must be the input itself (MSM_AMD_MLE_HIGH) or disjoint from all of it";
  return nullptr;
}

const char* fr_mle_eval_check(int scalar_layout, int order, const void* point, const void* in, uint64_t n, uint64_t n_vec,
                              uint64_t stride, const void* y_out, bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (n_vec == 0) return nullptr;
  if (const char* why = fr_mle_tables_check(n, n_vec, stride)) return why;
  if (!point || !in || !y_out) return "null pointer with work to do";
  if (device && ((uintptr_t)in & 15u)) return kMleAlign;
  return nullptr;
}

const char* fr_eq_table_check(int scalar_layout, int order, const void* point, uint64_t m, const void* out, bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (m < 1 || m > kFrMleMaxVars) return "m must be 1 .. 31";
  if (!point || !out) return "null pointer";
  if (device && ((uintptr_t)out & 15u)) return kMleAlign;
  return nullptr;
}

const char* fr_sumcheck_check(int scalar_layout, int order, int form, const void* in, uint64_t n, uint64_t n_vec,
                              uint64_t stride, const void* g_out, bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (form != kFrSumProduct && form != kFrSumEqAbC) return "form must be MSM_AMD_SUMCHECK_PRODUCT or MSM_AMD_SUMCHECK_EQ_AB_C";
  if (n_vec == 0) return nullptr;
  if (!fr_mle_degree(form, n_vec)) return "n_vec must be 1 .. 4 for MSM_AMD_SUMCHECK_PRODUCT and 4 for MSM_AMD_SUMCHECK_EQ_AB_C";
  if (const char* why = fr_mle_tables_check(n, n_vec, stride)) return why;
  if (!in || !g_out) return "null pointer with work to do";
  if (device && ((uintptr_t)in & 15u)) return kMleAlign;
  return nullptr;
}

static_assert(kFrSumMaxTables == MSM_AMD_SUMCHECK_MAX_TABLES && kFrSumMaxTerms == MSM_AMD_SUMCHECK_MAX_TERMS &&
              kFrSumMaxFactors == MSM_AMD_SUMCHECK_MAX_FACTORS && kFrSumNoOuter == MSM_AMD_SUMCHECK_NO_OUTER, "term lists");

const char* fr_sumcheck_terms_check(int scalar_layout, const ::msm_amd_fr_sumcheck_terms* terms, uint64_t n_vec,
                                    FrSumTerms* image) {
  if (!terms) return "null term list";
  if (n_vec < 1 || n_vec > kFrSumMaxTables) return "n_vec must be 1 .. 16 for a term list";
  if (terms->n_terms < 1 || terms->n_terms > kFrSumMaxTerms) return "n_terms must be 1 .. 16";
  if (!terms->coeff || !terms->term_len || !terms->factors) return "null pointer in the term list";
  if (terms->outer != kFrSumNoOuter && terms->outer >= n_vec)
    return "outer must be a table index below n_vec or MSM_AMD_SUMCHECK_NO_OUTER";
  uint32_t at = 0;
  for (uint32_t k = 0; k < terms->n_terms; ++k) {
    const uint32_t len = terms->term_len[k];
    if (len < 1 || len > kFrSumMaxFactors) return "a term length must be 1 .. 6";
    for (uint32_t j = 0; j < len; ++j)
      if (terms->factors[at + j] >= n_vec) return "a table index of a term is not below n_vec";
    at += len;
  }
  if (!image) return nullptr;
  *image = FrSumTerms{};
  image->n_terms = terms->n_terms, image->outer = terms->outer;
  const u256 one = Fr::one(), minus_one = Fr::sub(u256_zero(), one);
  auto same = [](const u256& a, const u256& b) {
    for (int i = 0; i < 8; ++i)
      if (a.v[i] != b.v[i]) return false;
    return true;
  };
  at = 0;
  for (uint32_t k = 0; k < terms->n_terms; ++k) {
    const u256 c = fr_read_record(scalar_layout, (const uint8_t*)terms->coeff + (size_t)k * 32);
    image->coeff[k] = c;
    fr_sum_set_byte(image->kind, k, same(c, one) ? kFrCoeffOne : same(c, minus_one) ? kFrCoeffMinusOne : kFrCoeffAny);
    fr_sum_set_byte(image->len, k, terms->term_len[k]);
    for (uint32_t j = 0; j < terms->term_len[k]; ++j) fr_sum_set_byte(image->idx, at + j, terms->factors[at + j]);
    at += terms->term_len[k];
  }
  return nullptr;
}

const char* fr_sumcheck_terms_round_check(int scalar_layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* in,
                                          uint64_t n, uint64_t n_vec, uint64_t stride, const void* g_out, bool device,
                                          FrSumTerms* image) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (n_vec == 0) return nullptr;
  if (const char* why = fr_sumcheck_terms_check(scalar_layout, terms, n_vec, image)) return why;
  if (const char* why = fr_mle_tables_check(n, n_vec, stride)) return why;
  if (!in || !g_out) return "null pointer with work to do";
  if (device && ((uintptr_t)in & 15u)) return kMleAlign;
  return nullptr;
}

const char* fr_sumcheck_step_check(int scalar_layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* r,
                                   const void* in, uint64_t n, uint64_t n_vec, uint64_t stride, const void* out,
                                   const void* g_out, bool device, FrSumTerms* image) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!fr_mle_order_known(order)) return kMleOrder;
  if (n_vec == 0) return nullptr;
  if (const char* why = fr_sumcheck_terms_check(scalar_layout, terms, n_vec, image)) return why;
  if (const char* why = fr_mle_tables_check(n, n_vec, stride)) return why;
  if (n < 4) return "n must be at least 4: the last variable is msm_amd_fr_mle_bind or msm_amd_fr_mle_eval";
  if (!r || !in || !out || !g_out) return "null pointer with work to do";
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return kMleAlign;
  if (out == in) return order == kFrMleHigh ? nullptr : "MSM_AMD_MLE_LOW is out of place only";
  if (!spans_apart(in, ((n_vec - 1) * stride + n) * 32, out, ((n_vec - 1) * stride + n / 2) * 32))
    return "the output must be the input itself (MSM_AMD_MLE_HIGH) or disjoint from all of it";
  return nullptr;
}

static_assert(kFrGateMaxCols == MSM_AMD_GATE_MAX_COLUMNS && kFrGateMaxTerms == MSM_AMD_GATE_MAX_TERMS &&
              kFrGateMaxFactors == MSM_AMD_GATE_MAX_FACTORS && kFrGateMaxOffsets == MSM_AMD_GATE_MAX_OFFSETS &&
              kFrGateMaxPeriod == MSM_AMD_GATE_MAX_PERIOD && kFrGateAccumulate == MSM_AMD_GATE_ACCUMULATE, "gates");

const char* fr_gate_terms_check(int scalar_layout, const ::msm_amd_fr_gate_terms* terms, uint64_t n_vec, uint64_t n,
                                uint64_t rot_step, FrGateTerms* image, bool coeffs) {
  if (!terms) return "null term list";
  if (n_vec < 1 || n_vec > kFrGateMaxCols) return "n_vec must be 1 .. 256 for a gate";
  if (n < 1 || (n >> 32)) return "n must be 1 .. 2^32 - 1";
  if (terms->n_terms < 1 || terms->n_terms > kFrGateMaxTerms) return "n_terms must be 1 .. 16";
  if (!terms->coeff || !terms->term_len || !terms->factors || !terms->rotations) return "null pointer in the term list";
  if (rot_step == 0) return "rot_step must be at least 1";
  FrGateTerms g{};
  g.n_terms = terms->n_terms;
  uint32_t at = 0;
  for (uint32_t k = 0; k < terms->n_terms; ++k) {
    const uint32_t len = terms->term_len[k];
    if (len < 1 || len > kFrGateMaxFactors) return "a term length must be 1 .. 8";
    for (uint32_t j = 0; j < len; ++j)
      if (terms->factors[at + j] >= n_vec) return "a column index of a term is not below n_vec";
    at += len;
  }
  at = 0;
  for (uint32_t k = 0; k < terms->n_terms; ++k) {
    fr_sum_set_byte(g.len, k, terms->term_len[k]);
    for (uint32_t j = 0; j < terms->term_len[k]; ++j, ++at) {
      // (rot rot_step) mod n, the non-negative remainder: |rot| <= 2^31 and rot_step < 2^64, so the product fits 128 bits
      const int64_t rot = terms->rotations[at];
      const unsigned __int128 mag = (unsigned __int128)(uint64_t)(rot < 0 ? -rot : rot) * rot_step;
      uint64_t off = (uint64_t)(mag % n);
      if (rot < 0 && off != 0) off = n - off;
      uint32_t s = 0;
      while (s < g.n_offsets && g.offset[s] != (uint32_t)off) ++s;
      if (s == g.n_offsets) {
        if (s == kFrGateMaxOffsets) return "more than MSM_AMD_GATE_MAX_OFFSETS (8) distinct offsets (rot * rot_step) mod n";
        g.offset[g.n_offsets++] = (uint32_t)off;
      }
      fr_sum_set_byte(g.col, at, terms->factors[at]);
      fr_sum_set_byte(g.slot, at, s);
    }
  }
  const u256 one = Fr::one(), minus_one = Fr::sub(u256_zero(), one);
  for (uint32_t k = 0; coeffs && k < terms->n_terms; ++k) {
    const u256 c = fr_read_record(scalar_layout, (const uint8_t*)terms->coeff + (size_t)k * 32);
    g.coeff[k] = c;
    fr_sum_set_byte(g.kind, k, u256_eq(c, one) ? kFrCoeffOne : u256_eq(c, minus_one) ? kFrCoeffMinusOne : kFrCoeffAny);
  }
  if (image) *image = g;
  return nullptr;
}

const char* fr_gate_eval_check(int mem, int scalar_layout, uint32_t flags, const ::msm_amd_fr_gate_terms* terms, const void* in,
                               uint64_t n, uint64_t n_vec, uint64_t stride, uint64_t rot_step, const void* k_acc32,
                               const void* scale, uint64_t period, const void* out, FrGateTerms* image) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE) return "mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE";
  if (flags & ~kFrGateAccumulate) return "flags must be 0 or MSM_AMD_GATE_ACCUMULATE";
  if (n >> 32) return "n >= 2^32";
  if (n == 0 || n_vec == 0) return nullptr;
  if (const char* why = fr_gate_terms_check(scalar_layout, terms, n_vec, n, rot_step, image, true)) return why;
  if (stride < n) return "stride < n";
  if ((stride >> 32) || ((n_vec * stride) >> 32)) return "n_vec * stride >= 2^32";
  if (!in || !out) return "null pointer with work to do";
  if ((flags & kFrGateAccumulate) && !k_acc32) return "null k_acc32 with MSM_AMD_GATE_ACCUMULATE";
  if (scale && (period < 1 || period > kFrGateMaxPeriod || (period & (period - 1)) || n % period))
    return "period must be a power of two, 1 .. 256, that divides n";
  if (mem == MSM_AMD_MEM_DEVICE && (((uintptr_t)in | (uintptr_t)out) & 15u)) return kMleAlign;
  if (!spans_apart(in, ((n_vec - 1) * stride + n) * 32, out, n * 32)) return "the output must be disjoint from all of the input";
  return nullptr;
}

namespace {

struct FrMatDictionary {
  std::vector<u256> records;
  static constexpr uint32_t kEmpty = 0xFFFFFFFFu;   // ids stay below it: nnz < 2^32
  std::vector<uint32_t> slots = std::vector<uint32_t>(1024, kEmpty);   // open addressing, a power of two
  static uint64_t hash(const u256& x) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int w = 0; w < 8; ++w) h = (h ^ x.v[w]) * 0xFF51AFD7ED558CCDull, h ^= h >> 29;
    return h;
  }
  static bool same(const u256& a, const u256& b) { return std::memcmp(a.v, b.v, 32) == 0; }
  void place(uint32_t id) {
    const size_t mask = slots.size() - 1;
    size_t at = hash(records[id]) & mask;
    while (slots[at] != kEmpty) at = (at + 1) & mask;
    slots[at] = id;
  }
  uint32_t id_of(const u256& x) {
    const size_t mask = slots.size() - 1;
    for (size_t at = hash(x) & mask;; at = (at + 1) & mask) {
      if (slots[at] == kEmpty) break;
      if (same(records[slots[at]], x)) return slots[at];
    }
    records.push_back(x);
    const uint32_t id = (uint32_t)(records.size() - 1);
    if (records.size() * 2 > slots.size()) {
      slots.assign(slots.size() * 2, kEmpty);
      for (uint32_t j = 0; j <= id; ++j) place(j);
    } else {
      place(id);
    }
    return id;
  }
};

}  // namespace

void fr_mat_build_image(int scalar_layout, uint64_t n_rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                        const void* values, uint32_t long_rows, uint32_t seg_log, FrMatPlan* plan, FrMatImage* at,
                        uint64_t* n_distinct, uint64_t* dict_records, std::vector<uint8_t>* image) {
  const uint64_t nnz = row_ptr[n_rows];
  std::vector<uint32_t> ids(nnz);
  FrMatDictionary dict;
  dict.id_of(Fr::one());                            // id 0
  dict.id_of(Fr::sub(u256_zero(), Fr::one()));      // id 1
  bool used[2] = {false, false};
  for (uint64_t k = 0; k < nnz; ++k) {
    ids[k] = dict.id_of(fr_read_record(scalar_layout, (const uint8_t*)values + k * 32));
    if (ids[k] < 2) used[ids[k]] = true;
  }
  std::vector<FrMatSeg> segs;
  std::vector<FrMatSplit> splits;
  *plan = fr_mat_plan(n_rows, row_ptr, long_rows, seg_log, &segs, &splits);
  *dict_records = dict.records.size();
  *n_distinct = *dict_records - (used[0] ? 0 : 1) - (used[1] ? 0 : 1);
  *at = fr_mat_image(n_rows, nnz, *dict_records, *plan);
  image->assign(at->bytes, 0);
  uint32_t* row_off = (uint32_t*)(image->data() + at->row_off);
  for (uint64_t i = 0; i <= n_rows; ++i) row_off[i] = (uint32_t)row_ptr[i];
  uint32_t* ent = (uint32_t*)(image->data() + at->ent);
  for (uint64_t k = 0; k < nnz; ++k) ent[2 * k] = col_idx[k], ent[2 * k + 1] = ids[k];
  std::memcpy(image->data() + at->dict, dict.records.data(), *dict_records * 32);
  if (!segs.empty()) std::memcpy(image->data() + at->segs, segs.data(), segs.size() * sizeof(FrMatSeg));
  if (!splits.empty()) std::memcpy(image->data() + at->splits, splits.data(), splits.size() * sizeof(FrMatSplit));
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

template <int OP>
void host_map_op(int layout, const u256& k, const uint8_t* a, const uint8_t* b, const uint8_t* c, size_t n, int threads,
                 uint8_t* out) {
  constexpr unsigned reads = fr_op_reads(OP);
  for_ranges(worker_count(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      const u256 x = host_get(layout, a, i);
      const u256 y = (reads & kFrReadsB) ? host_get(layout, b, i) : x;
      const u256 z = (reads & kFrReadsC) ? host_get(layout, c, i) : x;
      host_put(layout, out, i, fr_map_op<OP>(k, x, y, z));
    }
  });
}

int host_fr_map(int op, int layout, const void* k32, const void* a_v, const void* b_v, const void* c_v, size_t n, int threads,
                void* out_v) {
  if (fr_map_check(op, layout, k32, a_v, b_v, c_v, n, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  const u256 k = fr_read_k(op, layout, k32);
  const uint8_t *a = (const uint8_t*)a_v, *b = (const uint8_t*)b_v, *c = (const uint8_t*)c_v;
  uint8_t* out = (uint8_t*)out_v;
  switch (op) {
    case kFrAdd: host_map_op<kFrAdd>(layout, k, a, b, c, n, threads, out); break;
    case kFrSub: host_map_op<kFrSub>(layout, k, a, b, c, n, threads, out); break;
    case kFrMul: host_map_op<kFrMul>(layout, k, a, b, c, n, threads, out); break;
    case kFrScale: host_map_op<kFrScale>(layout, k, a, b, c, n, threads, out); break;
    case kFrAxpy: host_map_op<kFrAxpy>(layout, k, a, b, c, n, threads, out); break;
    default: host_map_op<kFrMulsubScale>(layout, k, a, b, c, n, threads, out); break;
  }
  return MSM_AMD_OK;
}

int host_fr_batch_inverse(int layout, const void* in_v, size_t n, int threads, void* out_v, uint64_t* n_zero) {
  if (n_zero) *n_zero = 0;
  if (fr_unary_check(layout, in_v, n, 1, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const unsigned T = worker_count(threads, n);
  std::vector<uint64_t> zeros(T, 0);
  for_ranges(T, n, [&](unsigned t, size_t lo, size_t hi) {
    if (lo >= hi) return;
    // before[i - lo] = the product of the non-zero records lo .. i - 1
    std::vector<u256> before(hi - lo);
    u256 acc = Fr::one();
    for (size_t i = lo; i < hi; ++i) {
      before[i - lo] = acc;
      const u256 x = host_get(layout, in, i);
      if (u256_is_zero(x)) ++zeros[t];
      else acc = Fr::mul(acc, x);
    }
    u256 inv = ntt_fr_inv(acc);   // of the product up to and including record i
    for (size_t i = hi; i-- > lo;) {
      const u256 x = host_get(layout, in, i);
      if (u256_is_zero(x)) {
        host_put(layout, out, i, x);
        continue;
      }
      host_put(layout, out, i, Fr::mul(inv, before[i - lo]));
      inv = Fr::mul(inv, x);
    }
  });
  if (n_zero)
    for (uint64_t z : zeros) *n_zero += z;
  return MSM_AMD_OK;
}

// SUM: the running sums of msm_amd_host_fr_prefix_sum (fr_scan_op); "product" below reads "sum" then
template <bool SUM>
int host_fr_prefix(int layout, int mode, const void* in_v, size_t n, size_t n_vec, int threads, void* out_v) {
  if (!fr_mode_known(mode) || fr_unary_check(layout, in_v, n, n_vec, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const size_t total = n * n_vec;
  const unsigned T = worker_count(threads, total);
  // phase 1: per range, the product of its records from the last start of a vector in it (or from its first record)
  std::vector<u256> tail(T, fr_scan_unit<SUM>());
  std::vector<char> restarts(T, 0);
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    u256 acc = fr_scan_unit<SUM>();
    for (size_t i = lo; i < hi; ++i) {
      if (i % n == 0) acc = fr_scan_unit<SUM>(), restarts[t] = 1;
      acc = fr_scan_op<SUM>(acc, host_get(layout, in, i));
    }
    tail[t] = acc;
  });
  // the product before the first record of every range
  std::vector<u256> carry(T, fr_scan_unit<SUM>());
  for (unsigned t = 1; t < T; ++t) carry[t] = restarts[t - 1] ? tail[t - 1] : fr_scan_op<SUM>(carry[t - 1], tail[t - 1]);
  // phase 2
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    u256 run = carry[t];
    for (size_t i = lo; i < hi; ++i) {
      if (i % n == 0) run = fr_scan_unit<SUM>();
      const u256 nxt = fr_scan_op<SUM>(run, host_get(layout, in, i));
      host_put(layout, out, i, mode == kFrInclusive ? nxt : run);
      run = nxt;
    }
  });
  return MSM_AMD_OK;
}

int host_fr_shift(int layout, const void* k32, const void* a_v, size_t n, int threads, void* out_v) {
  if (fr_shift_check(layout, k32, a_v, n, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  host_map_op<kFrShift>(layout, fr_read_record(layout, k32), (const uint8_t*)a_v, nullptr, nullptr, n, threads, (uint8_t*)out_v);
  return MSM_AMD_OK;
}

u256 host_pow(u256 base, uint64_t e) {
  u256 acc = Fr::one();
  for (; e != 0; e >>= 1) {
    if (e & 1) acc = Fr::mul(acc, base);
    base = Fr::mul(base, base);
  }
  return acc;
}

// The suffix sums s_i = sum_(j >= i) c_j z^(j - i) of n_vec vectors, the flat index space cut into T ranges.
// A range's first piece is what it holds of the vector its first record lies in.  Phase 1 leaves the Horner value of the
// first piece of every range that starts inside a vector; from them, last range first, s behind every range's last
// record.  Phase 2 walks every range down from there.  out null: the evaluation, one walk, which leaves the value of every
// piece that starts a vector and adds z^len s behind the range's last record to the one piece that a range end cuts.
int host_fr_poly(int layout, const void* z32, const void* in_v, size_t n, size_t n_vec, int threads, void* out_v, void* val_v,
                 bool divide) {
  if (fr_poly_check(layout, z32, in_v, n, n_vec, out_v, val_v, divide, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const u256 z = fr_read_record(layout, z32);
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t *out = (uint8_t*)out_v, *val = (uint8_t*)val_v;
  const size_t total = n * n_vec;
  const unsigned T = worker_count(threads, total);
  const size_t chunk = (total + T - 1) / T;
  auto lo_of = [&](unsigned t) { return std::min(total, t * chunk); };
  auto hi_of = [&](unsigned t) { return std::min(total, lo_of(t) + chunk); };
  auto piece_end = [&](size_t lo, size_t hi) { return std::min(hi, (lo / n + 1) * n); };   // of the first piece
  std::vector<u256> head(T, u256_zero()), behind(T, u256_zero()), value(divide ? 0 : n_vec, u256_zero());
  // phase 1
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    const size_t stop = divide ? (lo % n ? piece_end(lo, hi) : lo) : hi;
    u256 run = u256_zero();
    for (size_t i = stop; i-- > lo;) {
      run = Fr::add(Fr::mul(run, z), host_get(layout, in, i));
      if (i % n == 0) value[i / n] = run, run = u256_zero();
    }
    head[t] = run;
  });
  // s behind the last record of every range
  for (unsigned t = T - 1; t-- != 0;) {
    const size_t lo = lo_of(t + 1), hi = hi_of(t + 1);
    if (hi_of(t) % n == 0 || lo >= hi) continue;
    const size_t e = piece_end(lo, hi);
    behind[t] = e % n == 0 ? head[t + 1] : Fr::add(head[t + 1], Fr::mul(host_pow(z, e - lo), behind[t + 1]));
  }
  if (!divide) {
    for (unsigned t = 0; t < T; ++t) {
      const size_t hi = hi_of(t);
      if (hi % n == 0 || lo_of(t) >= hi || (hi - 1) / n * n < lo_of(t)) continue;   // the range end cuts a piece that starts a vector
      value[hi / n] = Fr::add(value[hi / n], Fr::mul(host_pow(z, hi % n), behind[t]));
    }
    for (size_t v = 0; v < n_vec; ++v) host_put(layout, val, v, value[v]);
    return MSM_AMD_OK;
  }
  // phase 2
  for_ranges(T, total, [&](unsigned t, size_t lo, size_t hi) {
    u256 run = behind[t];
    for (size_t i = hi; i-- > lo;) {
      if ((i + 1) % n == 0) run = u256_zero();
      const u256 c = host_get(layout, in, i);
      host_put(layout, out, i, run);
      run = Fr::add(Fr::mul(run, z), c);
      if (val && i % n == 0) host_put(layout, val, i / n, run);
    }
  });
  return MSM_AMD_OK;
}

// Upstream's shape (halo2 div_by_vanishing: roots.iter().fold(poly, kate_division)): the values from k evaluations of the
// input, then k chained divisions by X - z_j, the first from `in` to `out` and the others in place.  The values are
// gathered first and written last, so that an in-place call still evaluates the caller's polynomial.
int host_fr_poly_points(int layout, const void* z_v, size_t k, const void* in_v, size_t n, size_t n_vec, int threads, void* out_v,
                        void* val_v, bool divide) {
  if (fr_poly_points_check(MSM_AMD_MEM_HOST, layout, z_v, k, in_v, n, n_vec, out_v, val_v, divide)) return MSM_AMD_INPUT_ERROR;
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const uint8_t* z = (const uint8_t*)z_v;
  std::vector<uint8_t> vals(val_v ? k * n_vec * 32 : 0), y(n_vec * 32);
  if (val_v)
    for (size_t j = 0; j < k; ++j) {
      if (int rc = host_fr_poly(layout, z + j * 32, in_v, n, n_vec, threads, nullptr, y.data(), false)) return rc;
      for (size_t v = 0; v < n_vec; ++v) std::memcpy(vals.data() + (v * k + j) * 32, y.data() + v * 32, 32);
    }
  if (divide)
    for (size_t j = 0; j < k; ++j)
      if (int rc = host_fr_poly(layout, z + j * 32, j == 0 ? in_v : out_v, n, n_vec, threads, out_v, nullptr, true)) return rc;
  if (val_v) std::memcpy(val_v, vals.data(), vals.size());
  return MSM_AMD_OK;
}

int host_fr_lincomb(int layout, const void* k32, const void* a_v, size_t n, size_t n_vec, int threads, void* out_v) {
  if (fr_lincomb_check(layout, k32, a_v, n, n_vec, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const u256 k = fr_read_record(layout, k32);
  const uint8_t* a = (const uint8_t*)a_v;
  uint8_t* out = (uint8_t*)out_v;
  for_ranges(worker_count(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      u256 acc = host_get(layout, a, (n_vec - 1) * n + i);
      for (size_t v = n_vec - 1; v-- != 0;) acc = Fr::add(Fr::mul(acc, k), host_get(layout, a, v * n + i));
      host_put(layout, out, i, acc);
    }
  });
  return MSM_AMD_OK;
}

// Rows in T ranges of about equal entry count: range t starts at the first row whose offset reaches t nnz / T
int host_fr_matvec(int layout, uint64_t n_rows, uint64_t n_cols, const uint64_t* row_ptr, const uint32_t* col_idx,
                   const void* values_v, const void* x_v, int threads, void* y_v) {
  if (fr_matrix_check(layout, n_rows, n_cols, row_ptr, col_idx, values_v) || fr_matvec_check(layout, n_rows, n_cols, x_v, y_v, false))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t *values = (const uint8_t*)values_v, *x = (const uint8_t*)x_v;
  uint8_t* y = (uint8_t*)y_v;
  const uint64_t nnz = row_ptr[n_rows];
  const unsigned T = worker_count(threads, n_rows);
  std::vector<uint64_t> start(T + 1, n_rows);
  start[0] = 0;
  for (unsigned t = 1; t < T; ++t)
    start[t] = std::lower_bound(row_ptr, row_ptr + n_rows, nnz / T * t + nnz % T * t / T) - row_ptr;
  for_ranges(T, T, [&](unsigned, size_t lo, size_t hi) {
    for (size_t t = lo; t < hi; ++t)
      for (uint64_t i = start[t]; i < start[t + 1]; ++i) {
        u256 acc = u256_zero();
        for (uint64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
          acc = Fr::add(acc, Fr::mul(host_get(layout, values, k), host_get(layout, x, col_idx[k])));
        host_put(layout, y, i, acc);
      }
  });
  return MSM_AMD_OK;
}

// ---- multilinear tables (fr_mle.hip.h) -------------------------------------------------------------------------------------
// a call's work is cut into ranges of at least 2^10 items, so that a short table starts no thread
unsigned mle_workers(int threads, uint64_t items) { return worker_count(threads, (size_t)((items + 1023) >> 10)); }

// n_bind steps of `order` on one table of n records: what is left, as Montgomery residues
std::vector<u256> host_mle_fold(int layout, int order, const u256* r, uint32_t n_bind, const uint8_t* tab, uint64_t n, int threads) {
  std::vector<u256> cur, nxt;
  uint64_t len = n;
  for (uint32_t s = 0; s < n_bind; ++s) {
    const uint64_t h = len / 2;
    nxt.resize(h);
    for_ranges(mle_workers(threads, h), h, [&](unsigned, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const size_t a = order == kFrMleHigh ? i : 2 * i, b = order == kFrMleHigh ? i + h : 2 * i + 1;
        nxt[i] = s == 0 ? fr_mle_fold(host_get(layout, tab, a), host_get(layout, tab, b), r[0]) : fr_mle_fold(cur[a], cur[b], r[s]);
      }
    });
    cur.swap(nxt);
    len = h;
  }
  return cur;
}

void host_read_records(int layout, const void* src, uint64_t count, u256* dst) {
  for (uint64_t j = 0; j < count; ++j) dst[j] = fr_read_record(layout, (const uint8_t*)src + j * 32);
}

int host_fr_mle_bind(int layout, int order, const void* r32, size_t n_bind, const void* in_v, size_t n, size_t n_vec,
                     size_t stride, int threads, void* out_v) {
  if (fr_mle_bind_check(layout, order, r32, n_bind, in_v, n, n_vec, stride, out_v, false)) return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  u256 r[kFrMleMaxVars];
  host_read_records(layout, r32, n_bind, r);
  for (size_t v = 0; v < n_vec; ++v) {
    const std::vector<u256> left = host_mle_fold(layout, order, r, (uint32_t)n_bind, (const uint8_t*)in_v + v * stride * 32, n, threads);
    for (size_t i = 0; i < left.size(); ++i) host_put(layout, (uint8_t*)out_v + v * stride * 32, i, left[i]);
  }
  return MSM_AMD_OK;
}

int host_fr_mle_eval(int layout, int order, const void* point32, const void* in_v, size_t n, size_t n_vec, size_t stride,
                     int threads, void* y_out) {
  if (fr_mle_eval_check(layout, order, point32, in_v, n, n_vec, stride, y_out, false)) return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  const uint32_t m = fr_mle_log2(n);
  u256 r[kFrMleMaxVars];
  host_read_records(layout, point32, m, r);
  for (size_t v = 0; v < n_vec; ++v)
    host_put(layout, (uint8_t*)y_out, v, host_mle_fold(layout, order, r, m, (const uint8_t*)in_v + v * stride * 32, n, threads)[0]);
  return MSM_AMD_OK;
}

// out[i] = lo[i mod 2^k] hi[i / 2^k]: the factors of the lower and of the upper bits, one product per output
int host_fr_eq_table(int layout, int order, const void* point32, size_t m, int threads, void* out_v) {
  if (fr_eq_table_check(layout, order, point32, m, out_v, false)) return MSM_AMD_INPUT_ERROR;
  u256 p[kFrMleMaxVars], by_bit[kFrMleMaxVars];
  host_read_records(layout, point32, m, p);
  for (size_t b = 0; b < m; ++b) by_bit[b] = p[order == kFrMleHigh ? m - 1 - b : b];
  auto table = [&](uint32_t first, uint32_t bits) {
    std::vector<u256> t(1, Fr::one());
    for (uint32_t b = 0; b < bits; ++b) {
      const u256 one_less = Fr::sub(Fr::one(), by_bit[first + b]);
      t.resize(t.size() * 2);
      for (size_t i = t.size() / 2; i-- != 0;) t[i + t.size() / 2] = Fr::mul(t[i], by_bit[first + b]), t[i] = Fr::mul(t[i], one_less);
    }
    return t;
  };
  const uint32_t k = (uint32_t)m / 2;
  const std::vector<u256> lo = table(0, k), hi = table(k, (uint32_t)m - k);
  const uint64_t n = (uint64_t)1 << m;
  for_ranges(mle_workers(threads, n), n, [&](unsigned, size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) host_put(layout, (uint8_t*)out_v, i, Fr::mul(lo[i & ((1u << k) - 1)], hi[i >> k]));
  });
  return MSM_AMD_OK;
}

template <int FORM, int K>
void host_round_form(int layout, int order, const uint8_t* in, uint64_t n, uint64_t stride, int threads, u256* g) {
  using Sums = FrMleSums<FORM, K>;
  const uint64_t h = n / 2;
  const unsigned T = mle_workers(threads, h);
  std::vector<Sums> part(T);
  for_ranges(T, h, [&](unsigned t, size_t a, size_t b) {
    Sums s;
    s.clear();
    for (size_t x = a; x < b; ++x) {
      u256 lo[K], hi[K];
      for (int j = 0; j < K; ++j) {
        lo[j] = host_get(layout, in + j * stride * 32, order == kFrMleHigh ? x : 2 * x);
        hi[j] = host_get(layout, in + j * stride * 32, order == kFrMleHigh ? x + h : 2 * x + 1);
      }
      s.add_pair(lo, hi);
    }
    part[t] = s;
  });
  for (int v = 0; v < Sums::kValues; ++v) {
    g[v] = u256_zero();
    for (unsigned t = 0; t < T; ++t) g[v] = Fr::add(g[v], part[t].g[v]);
  }
}

int host_fr_sumcheck_round(int layout, int order, int form, const void* in_v, size_t n, size_t n_vec, size_t stride, int threads,
                           void* g_out) {
  if (fr_sumcheck_check(layout, order, form, in_v, n, n_vec, stride, g_out, false)) return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  const uint8_t* in = (const uint8_t*)in_v;
  u256 g[kFrMleMaxValues];
  if (form == kFrSumEqAbC) host_round_form<kFrSumEqAbC, 4>(layout, order, in, n, stride, threads, g);
  else if (n_vec == 1) host_round_form<kFrSumProduct, 1>(layout, order, in, n, stride, threads, g);
  else if (n_vec == 2) host_round_form<kFrSumProduct, 2>(layout, order, in, n, stride, threads, g);
  else if (n_vec == 3) host_round_form<kFrSumProduct, 3>(layout, order, in, n, stride, threads, g);
  else host_round_form<kFrSumProduct, 4>(layout, order, in, n, stride, threads, g);
  for (uint32_t t = 0; t <= fr_mle_degree(form, n_vec); ++t) host_put(layout, (uint8_t*)g_out, t, g[t]);
  return MSM_AMD_OK;
}

// the same body over ranges of pairs, the sums of the ranges added in range order
template <int V>
void host_terms_values(const FrSumTerms& terms, int layout, int order, const uint8_t* in, uint64_t n, uint64_t stride, int threads,
                       u256* g) {
  const uint64_t h = n / 2;
  const unsigned T = mle_workers(threads, h);
  std::vector<FrTermSums<V>> part(T);
  for_ranges(T, h, [&](unsigned t, size_t a, size_t b) {
    FrTermSums<V> s;
    s.clear();
    for (size_t x = a; x < b; ++x)
      s.add_pair(terms, [&](uint32_t v, u256& lo, u256& hi) {
        lo = host_get(layout, in + (size_t)v * stride * 32, order == kFrMleHigh ? x : 2 * x);
        hi = host_get(layout, in + (size_t)v * stride * 32, order == kFrMleHigh ? x + h : 2 * x + 1);
      });
    part[t] = s;
  });
  for (int v = 0; v < V; ++v) {
    g[v] = u256_zero();
    for (unsigned t = 0; t < T; ++t) g[v] = Fr::add(g[v], part[t].g[v]);
  }
}

void host_terms_round(const FrSumTerms& terms, int layout, int order, const uint8_t* in, uint64_t n, uint64_t stride, int threads,
                      void* g_out) {
  u256 g[kFrSumMaxValues];
  const uint32_t d = fr_sum_degree(terms);
  switch (d) {
    case 1: host_terms_values<2>(terms, layout, order, in, n, stride, threads, g); break;
    case 2: host_terms_values<3>(terms, layout, order, in, n, stride, threads, g); break;
    case 3: host_terms_values<4>(terms, layout, order, in, n, stride, threads, g); break;
    case 4: host_terms_values<5>(terms, layout, order, in, n, stride, threads, g); break;
    case 5: host_terms_values<6>(terms, layout, order, in, n, stride, threads, g); break;
    case 6: host_terms_values<7>(terms, layout, order, in, n, stride, threads, g); break;
    default: host_terms_values<8>(terms, layout, order, in, n, stride, threads, g); break;
  }
  for (uint32_t t = 0; t <= d; ++t) host_put(layout, (uint8_t*)g_out, t, g[t]);
}

int host_fr_sumcheck_round_terms(int layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* in_v, size_t n,
                                 size_t n_vec, size_t stride, int threads, void* g_out) {
  FrSumTerms image;
  if (fr_sumcheck_terms_round_check(layout, order, terms, in_v, n, n_vec, stride, g_out, false, &image)) return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  host_terms_round(image, layout, order, (const uint8_t*)in_v, n, stride, threads, g_out);
  return MSM_AMD_OK;
}

// bind, then the round over what the bind wrote: the definition of the step
int host_fr_sumcheck_step_terms(int layout, int order, const ::msm_amd_fr_sumcheck_terms* terms, const void* r32, const void* in_v,
                                size_t n, size_t n_vec, size_t stride, int threads, void* out_v, void* g_out) {
  FrSumTerms image;
  if (fr_sumcheck_step_check(layout, order, terms, r32, in_v, n, n_vec, stride, out_v, g_out, false, &image))
    return MSM_AMD_INPUT_ERROR;
  if (n_vec == 0) return MSM_AMD_OK;
  const u256 r = fr_read_record(layout, r32);
  for (size_t v = 0; v < n_vec; ++v) {
    const std::vector<u256> left = host_mle_fold(layout, order, &r, 1, (const uint8_t*)in_v + v * stride * 32, n, threads);
    for (size_t i = 0; i < left.size(); ++i) host_put(layout, (uint8_t*)out_v + v * stride * 32, i, left[i]);
  }
  host_terms_round(image, layout, order, (const uint8_t*)out_v, n / 2, stride, threads, g_out);
  return MSM_AMD_OK;
}

// the calls of a gate that have no ctx leave their refusal here
thread_local const char* gate_why = "";

// the body of fr_gate_kernel row by row over ranges of rows
int host_fr_gate_eval(int layout, uint32_t flags, const ::msm_amd_fr_gate_terms* terms, const void* in_v, size_t n, size_t n_vec,
                      size_t stride, uint64_t rot_step, const void* k_acc32, const void* scale_v, size_t period, int threads,
                      void* out_v) {
  FrGateTerms image;
  gate_why = "";
  if (const char* why = fr_gate_eval_check(MSM_AMD_MEM_HOST, layout, flags, terms, in_v, n, n_vec, stride, rot_step, k_acc32,
                                           scale_v, period, out_v, &image)) {
    gate_why = why;
    return MSM_AMD_INPUT_ERROR;
  }
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const bool accumulate = flags & kFrGateAccumulate;
  const u256 k_acc = accumulate ? fr_read_record(layout, k_acc32) : u256_zero();
  std::vector<u256> scale(scale_v ? period : 0);
  if (scale_v) host_read_records(layout, scale_v, period, scale.data());
  for_ranges(worker_count(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      u256 v = fr_gate_row(image, i, n, [&](uint32_t col, uint64_t row) { return host_get(layout, in + (size_t)col * stride * 32, row); });
      if (accumulate) v = Fr::add(Fr::mul(k_acc, host_get(layout, out, i)), v);
      if (scale_v) v = Fr::mul(v, scale[i & (period - 1)]);
      host_put(layout, out, i, v);
    }
  });
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_host_fr_mle_bind(int scalar_layout, int order, const void* r, size_t n_bind, const void* in, size_t n, size_t n_vec,
                             size_t stride, int threads, void* out) {
  return msm_amd::host_fr_mle_bind(scalar_layout, order, r, n_bind, in, n, n_vec, stride, threads, out);
}

int msm_amd_host_fr_mle_eval(int scalar_layout, int order, const void* point, const void* in, size_t n, size_t n_vec,
                             size_t stride, int threads, void* y_out) {
  return msm_amd::host_fr_mle_eval(scalar_layout, order, point, in, n, n_vec, stride, threads, y_out);
}

int msm_amd_host_fr_eq_table(int scalar_layout, int order, const void* point, size_t m, int threads, void* out) {
  return msm_amd::host_fr_eq_table(scalar_layout, order, point, m, threads, out);
}

int msm_amd_host_fr_sumcheck_round(int scalar_layout, int order, int form, const void* in, size_t n, size_t n_vec, size_t stride,
                                   int threads, void* g_out) {
  return msm_amd::host_fr_sumcheck_round(scalar_layout, order, form, in, n, n_vec, stride, threads, g_out);
}

int msm_amd_test_fr_mle_plan(int call, int order, int form, size_t n, size_t n_vec, uint32_t n_bind, uint32_t chunk_log,
                             uint32_t tile_log, uint64_t counts[8]) {
  using namespace msm_amd;
  if (!counts || chunk_log < kFrMleMinChunkLog || chunk_log > kFrMleMaxChunkLog || tile_log < kFrMinTileLog ||
      tile_log > kFrTileLog || !fr_mle_order_known(order))
    return MSM_AMD_INPUT_ERROR;
  uint64_t c[8] = {};
  if (call == MSM_AMD_MLE_CALL_EQ_TABLE) {   // n is m
    if (n < 1 || n > kFrMleMaxVars) return MSM_AMD_INPUT_ERROR;
    const uint64_t lanes = (uint64_t)1 << (n >= kFrMleEqWideFrom ? n - kFrMleEqSpread : n);
    c[0] = 1, c[1] = (lanes + kFrWave - 1) / kFrWave, c[6] = (uint64_t)1 << n;
  } else {
    if (n_vec == 0 || fr_mle_tables_check(n, n_vec, n)) return MSM_AMD_INPUT_ERROR;
    if (call == MSM_AMD_MLE_CALL_BIND) {
      if (n_bind == 0 || n_bind > fr_mle_log2(n)) return MSM_AMD_INPUT_ERROR;
      const FrMleBindPlan p = fr_mle_bind_plan(order, n, n_vec, n_bind);
      c[0] = p.launches, c[1] = p.waves, c[2] = p.work_records, c[4] = p.launches, c[6] = (n >> n_bind) * n_vec;
    } else if (call == MSM_AMD_MLE_CALL_EVAL) {
      const FrScanPlan p = fr_scan_plan(n, n_vec, tile_log);
      c[0] = p.levels, c[2] = p.records + n_vec, c[4] = p.levels, c[5] = p.tiles[0] * n_vec, c[6] = n_vec;
      for (uint32_t k = 0; k < p.levels; ++k) c[1] += p.tiles[k] * n_vec;
    } else if (call == MSM_AMD_MLE_CALL_ROUND) {
      const uint32_t d = fr_mle_degree(form, n_vec);
      if (!d) return MSM_AMD_INPUT_ERROR;
      const FrMleRoundPlan p = fr_mle_round_plan(n, d + 1, chunk_log);
      c[0] = p.launches, c[1] = p.waves, c[2] = p.records, c[4] = p.levels, c[5] = p.count[0], c[6] = p.values;
    } else {
      return MSM_AMD_INPUT_ERROR;
    }
  }
  c[3] = c[2] * 32;
  std::memcpy(counts, c, sizeof c);
  return MSM_AMD_OK;
}

int msm_amd_fr_sumcheck_terms_degree(const msm_amd_fr_sumcheck_terms* terms, size_t n_vec, uint32_t* d) {
  using namespace msm_amd;
  if (!d || fr_sumcheck_terms_check(MSM_AMD_SCALAR_MONT_LE, terms, n_vec, nullptr)) return MSM_AMD_INPUT_ERROR;
  uint32_t longest = 0;
  for (uint32_t k = 0; k < terms->n_terms; ++k) longest = terms->term_len[k] > longest ? terms->term_len[k] : longest;
  *d = longest + (terms->outer != kFrSumNoOuter ? 1u : 0u);
  return MSM_AMD_OK;
}

int msm_amd_host_fr_sumcheck_round_terms(int scalar_layout, int order, const msm_amd_fr_sumcheck_terms* terms, const void* in,
                                         size_t n, size_t n_vec, size_t stride, int threads, void* g_out) {
  return msm_amd::host_fr_sumcheck_round_terms(scalar_layout, order, terms, in, n, n_vec, stride, threads, g_out);
}

int msm_amd_host_fr_sumcheck_step_terms(int scalar_layout, int order, const msm_amd_fr_sumcheck_terms* terms, const void* r,
                                        const void* in, size_t n, size_t n_vec, size_t stride, int threads, void* out,
                                        void* g_out) {
  return msm_amd::host_fr_sumcheck_step_terms(scalar_layout, order, terms, r, in, n, n_vec, stride, threads, out, g_out);
}

int msm_amd_test_fr_sumcheck_terms_plan(const msm_amd_fr_sumcheck_terms* terms, size_t n, size_t n_vec, uint32_t chunk_log,
                                        int step, uint64_t counts[8]) {
  using namespace msm_amd;
  uint32_t d = 0;
  if (!counts || chunk_log < kFrMleMinChunkLog || chunk_log > kFrMleMaxChunkLog ||
      msm_amd_fr_sumcheck_terms_degree(terms, n_vec, &d) != MSM_AMD_OK || fr_mle_tables_check(n, n_vec, n) || (step && n < 4))
    return MSM_AMD_INPUT_ERROR;
  const FrMleRoundPlan p = fr_mle_round_plan(step ? n / 2 : n, d + 1, chunk_log);
  const uint64_t c[8] = {p.launches, p.waves, p.records, p.records * 32, p.levels, p.count[0], p.values, 0};
  std::memcpy(counts, c, sizeof c);
  return MSM_AMD_OK;
}

int msm_amd_fr_gate_check(const msm_amd_fr_gate_terms* terms, size_t n_vec, size_t n, uint64_t rot_step, uint32_t* degree,
                          uint32_t* n_offsets) {
  using namespace msm_amd;
  FrGateTerms image;
  gate_why = "";
  if (const char* why = fr_gate_terms_check(MSM_AMD_SCALAR_MONT_LE, terms, n_vec, n, rot_step, &image, false)) {
    gate_why = why;
    return MSM_AMD_INPUT_ERROR;
  }
  if (degree) *degree = fr_gate_degree(image);
  if (n_offsets) *n_offsets = image.n_offsets;
  return MSM_AMD_OK;
}

const char* msm_amd_fr_gate_last_error(void) { return msm_amd::gate_why; }

int msm_amd_host_fr_gate_eval(int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms, const void* in, size_t n,
                              size_t n_vec, size_t stride, uint64_t rot_step, const void* k_acc32, const void* scale,
                              size_t period, int threads, void* out) {
  return msm_amd::host_fr_gate_eval(scalar_layout, flags, terms, in, n, n_vec, stride, rot_step, k_acc32, scale, period, threads,
                                    out);
}

int msm_amd_test_fr_gate_plan(int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms, size_t n, size_t n_vec,
                              uint64_t rot_step, size_t period, uint64_t counts[8]) {
  using namespace msm_amd;
  FrGateTerms g;
  gate_why = "";
  const char* why = !counts                              ? "null counts"
                    : !fr_layout_known(scalar_layout)    ? "scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only"
                    : (flags & ~kFrGateAccumulate)       ? "flags must be 0 or MSM_AMD_GATE_ACCUMULATE"
                                                         : fr_gate_terms_check(scalar_layout, terms, n_vec, n, rot_step, &g, true);
  if (!why && period && (period > kFrGateMaxPeriod || (period & (period - 1)) || n % period))
    why = "period must be a power of two, 1 .. 256, that divides n";
  if (why) {
    gate_why = why;
    return MSM_AMD_INPUT_ERROR;
  }
  const uint64_t extra = (flags & kFrGateAccumulate ? 1u : 0u) + (period ? 1u : 0u);
  const uint64_t c[8] = {1, ((uint64_t)n + kFrMapThreads - 1) / kFrMapThreads, fr_gate_factors(g) + extra,
                         fr_gate_products(g) + extra, g.n_offsets, (uint64_t)period * 32, fr_gate_degree(g), 0};
  std::memcpy(counts, c, sizeof c);
  return MSM_AMD_OK;
}

int msm_amd_host_fr_matvec(int scalar_layout, size_t n_rows, size_t n_cols, const uint64_t* row_ptr, const uint32_t* col_idx,
                           const void* values, const void* x, int threads, void* y) {
  return msm_amd::host_fr_matvec(scalar_layout, n_rows, n_cols, row_ptr, col_idx, values, x, threads, y);
}

int msm_amd_test_fr_matrix_plan(size_t n_rows, const uint64_t* row_ptr, uint32_t long_rows, uint32_t seg_log,
                                uint64_t counts[8], uint32_t* segs, size_t segs_cap) {
  using namespace msm_amd;
  const uint64_t rows = n_rows;
  if (!counts || !row_ptr || rows == 0 || (rows >> 32) || long_rows < kFrMatMinLong || long_rows > kFrMatMaxLong ||
      seg_log < kFrMatMinSegLog || seg_log > kFrMatMaxSegLog || (segs_cap && !segs) || row_ptr[0] != 0)
    return MSM_AMD_INPUT_ERROR;
  for (uint64_t i = 0; i < rows; ++i)
    if (row_ptr[i + 1] < row_ptr[i] || (row_ptr[i + 1] >> 32)) return MSM_AMD_INPUT_ERROR;
  std::vector<FrMatSeg> all;
  const FrMatPlan p = fr_mat_plan(rows, row_ptr, long_rows, seg_log, &all, nullptr);
  const uint64_t c[8] = {p.lane_rows, p.wave_rows, p.segments, p.split_rows, p.partials, p.launches, p.waves, 0};
  std::memcpy(counts, c, sizeof c);
  const size_t take = std::min<size_t>(segs_cap, all.size());
  if (take) std::memcpy(segs, all.data(), take * sizeof(FrMatSeg));
  return MSM_AMD_OK;
}

int msm_amd_host_fr_poly_eval(int scalar_layout, const void* z32, const void* coeffs, size_t n, size_t n_vec, int threads,
                              void* y_out) {
  return msm_amd::host_fr_poly(scalar_layout, z32, coeffs, n, n_vec, threads, nullptr, y_out, false);
}

int msm_amd_host_fr_poly_div_linear(int scalar_layout, const void* z32, const void* in, size_t n, size_t n_vec, int threads,
                                    void* out, void* rem_out) {
  return msm_amd::host_fr_poly(scalar_layout, z32, in, n, n_vec, threads, out, rem_out, true);
}

int msm_amd_host_fr_poly_eval_points(int scalar_layout, const void* z, size_t k, const void* coeffs, size_t n, size_t n_vec,
                                     int threads, void* y_out) {
  return msm_amd::host_fr_poly_points(scalar_layout, z, k, coeffs, n, n_vec, threads, nullptr, y_out, false);
}

int msm_amd_host_fr_poly_div_points(int scalar_layout, const void* z, size_t k, const void* in, size_t n, size_t n_vec,
                                    int threads, void* out, void* vals_out) {
  return msm_amd::host_fr_poly_points(scalar_layout, z, k, in, n, n_vec, threads, out, vals_out, true);
}

int msm_amd_test_fr_poly_points_plan(size_t n, size_t n_vec, size_t k, uint32_t tile_log, int divide, uint64_t counts[8]) {
  using namespace msm_amd;
  const uint64_t n64 = n, v64 = n_vec;
  if (!counts || tile_log < kFrMinTileLog || tile_log > kFrTileLog || k == 0 || k > kFrPolyMaxPoints || n == 0 || n_vec == 0 ||
      (n64 >> 32) || (v64 >> 32) || ((n64 * v64) >> 32))
    return MSM_AMD_INPUT_ERROR;
  const FrScanPlan p = fr_scan_plan(n, n_vec, tile_log);
  // level 0 runs all k points in one wave per tile, a level above one wave per point and tile; a division reduces every
  // level but the top one and scans every level
  uint64_t waves = 0;
  for (uint32_t l = 0; l < p.levels; ++l) {
    const uint64_t w = p.tiles[l] * n_vec * (l == 0 ? 1 : k);
    waves += divide ? (l + 1 < p.levels ? 2 * w : w) : w;
  }
  const uint64_t records = fr_poly_points_records(p, n_vec, k);
  const uint64_t level0 = p.tiles[0] * n_vec * (divide && p.levels > 1 ? 2 : 1);
  const uint64_t c[8] = {divide ? p.launches : p.levels, waves, records, records * 32, p.levels, sizeof(FrPolyPointsArgs), level0, 0};
  std::memcpy(counts, c, sizeof c);
  return MSM_AMD_OK;
}

int msm_amd_host_fr_lincomb(int scalar_layout, const void* k32, const void* a, size_t n, size_t n_vec, int threads, void* out) {
  return msm_amd::host_fr_lincomb(scalar_layout, k32, a, n, n_vec, threads, out);
}

int msm_amd_host_fr_map(int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c, size_t n,
                        int threads, void* out) {
  return msm_amd::host_fr_map(op, scalar_layout, k32, a, b, c, n, threads, out);
}

int msm_amd_host_fr_batch_inverse(int scalar_layout, const void* in, size_t n, int threads, void* out, uint64_t* n_zero) {
  return msm_amd::host_fr_batch_inverse(scalar_layout, in, n, threads, out, n_zero);
}

int msm_amd_host_fr_prefix_product(int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, int threads,
                                   void* out) {
  return msm_amd::host_fr_prefix<false>(scalar_layout, mode, in, n, n_vec, threads, out);
}

int msm_amd_host_fr_prefix_sum(int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, int threads, void* out) {
  return msm_amd::host_fr_prefix<true>(scalar_layout, mode, in, n, n_vec, threads, out);
}

int msm_amd_host_fr_shift(int scalar_layout, const void* k32, const void* a, size_t n, int threads, void* out) {
  return msm_amd::host_fr_shift(scalar_layout, k32, a, n, threads, out);
}

int msm_amd_test_fr_plan(size_t n, size_t n_vec, uint32_t tile_log, uint64_t out[4]) {
  using namespace msm_amd;
  const uint64_t n64 = n, v64 = n_vec;
  if (!out || tile_log < kFrMinTileLog || tile_log > kFrTileLog || (n64 >> 32) || (v64 >> 32) || ((n64 * v64) >> 32))
    return MSM_AMD_INPUT_ERROR;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const FrScanPlan p = fr_scan_plan(n, n_vec, tile_log);
  out[0] = p.levels, out[1] = p.launches, out[2] = p.tiles[0] * n_vec, out[3] = p.records;
  return MSM_AMD_OK;
}

}  // extern "C"

// ---- Poseidon (fr_poseidon.hip.h): the checks, the constants of the reference generator, the twins ---------------------------
namespace msm_amd {

const char* poseidon_shape_check(uint64_t t, uint64_t r_f, uint64_t r_p) {
  if (t < kPoseidonMinT || t > kPoseidonMaxT) return "t must be 2 .. 5";
  if (r_f == 0 || (r_f & 1u)) return "r_f must be even and at least 2";
  if (r_f > kPoseidonMaxRounds || r_p > kPoseidonMaxRounds || r_f + r_p > kPoseidonMaxRounds) return "r_f + r_p > 128";
  return nullptr;
}

const char* poseidon_constants_check(uint64_t t, uint64_t r_f, uint64_t r_p, int scalar_layout, const void* ark, const void* mds) {
  if (const char* why = poseidon_shape_check(t, r_f, r_p)) return why;
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (!ark || !mds) return "null ark or mds";
  return nullptr;
}

const char* poseidon_call_check(int kind, uint32_t t, int scalar_layout, const void* in, uint64_t n, const void* out, bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (n >> 32) return "n >= 2^32";
  if (n == 0) return nullptr;
  if (!in || !out) return "null pointer with n > 0";
  if (device && (((uintptr_t)in | (uintptr_t)out) & 15u)) return kMleAlign;
  const uint64_t in_bytes = n * (kind == kPoseidonHash ? t - 1 : t) * 32, out_bytes = n * (kind == kPoseidonHash ? 1 : t) * 32;
  if (kind == kPoseidonPermute || t == 2)
    return fr_overlap_ok(out, in, in_bytes) ? nullptr : "the output must be the input itself or disjoint from it";
  // digest i would land on a record that the lane of group i / (t - 1) reads, and nothing orders two workgroups
  return spans_apart(in, in_bytes, out, out_bytes) ? nullptr : "with t >= 3 the digests must be disjoint from the input";
}

const char* poseidon_merkle_check(uint32_t t, int scalar_layout, const void* leaves, uint64_t n_leaves, const void* tree,
                                  bool device) {
  if (!fr_layout_known(scalar_layout)) return kMleLayout;
  if (t < 3) return "a tree needs t >= 3: its arity is t - 1";
  if ((n_leaves >> 32) || !poseidon_tree_depth(n_leaves, t - 1)) return "n_leaves must be (t - 1)^d, d >= 1, below 2^32";
  if (!leaves || !tree) return "null leaves or tree";
  if (device && (((uintptr_t)leaves | (uintptr_t)tree) & 15u)) return kMleAlign;
  if (!spans_apart(leaves, n_leaves * 32, tree, (n_leaves - 1) / (t - 2) * 32)) return "the tree must not overlap the leaves";
  return nullptr;
}

const char* poseidon_paths_check(uint32_t t, int scalar_layout, const void* leaves, uint64_t n_leaves, const void* tree,
                                 const uint64_t* idx, uint64_t n_idx, const void* out, bool device) {
  if (const char* why = poseidon_merkle_check(t, scalar_layout, leaves, n_leaves, tree, device)) return why;
  const uint64_t per = (uint64_t)poseidon_tree_depth(n_leaves, t - 1) * (t - 2);
  if ((n_idx >> 32) || ((n_idx * per) >> 32)) return "n_idx * d * (t - 2) >= 2^32";
  if (n_idx == 0) return nullptr;
  if (!idx || !out) return "null idx or out with n_idx > 0";
  if (device && ((uintptr_t)out & 15u)) return kMleAlign;
  for (uint64_t k = 0; k < n_idx; ++k)
    if (idx[k] >= n_leaves) return "a leaf index is not below n_leaves";
  if (!spans_apart(leaves, n_leaves * 32, out, n_idx * per * 32) ||
      !spans_apart(tree, (n_leaves - 1) / (t - 2) * 32, out, n_idx * per * 32))
    return "the paths must not overlap the leaves or the tree";
  return nullptr;
}

void poseidon_build_image(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                          std::vector<u256>* image) {
  const uint32_t rounds = r_f + r_p;
  image->assign(poseidon_image_records(t, rounds), u256_zero());
  for (uint32_t k = 0; k < poseidon_ark_records(t, rounds); ++k) (*image)[k] = fr_read_record(scalar_layout, (const uint8_t*)ark + k * 32);
  for (uint32_t k = 0; k < t * t; ++k) (*image)[poseidon_mds_at(t, rounds) + k] = fr_read_record(scalar_layout, (const uint8_t*)mds + k * 32);
}

namespace {

// The Grain LFSR of the Poseidon paper's generate_parameters_grain: 80 bits, the fields most significant bit first
struct PoseidonGrain {
  uint8_t s[80];
  PoseidonGrain(uint32_t t, uint32_t r_f, uint32_t r_p) {
    int at = 0;
    auto field = [&](uint32_t value, int bits) {
      for (int b = bits - 1; b >= 0; --b) s[at++] = (value >> b) & 1u;
    };
    field(1, 2), field(0, 4), field(254, 12), field(t, 12), field(r_f, 10), field(r_p, 10);
    while (at < 80) s[at++] = 1;
    for (int k = 0; k < 160; ++k) update();
  }
  uint8_t update() {
    const uint8_t b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0];
    std::memmove(s, s + 1, 79);
    s[79] = b;
    return b;
  }
  uint8_t bit() {
    uint8_t first = update();
    while (!first) update(), first = update();
    return update();
  }
  u256 integer() {   // 254 bits, the first one most significant
    u256 x = u256_zero();
    for (int b = 253; b >= 0; --b) x.v[b >> 5] |= (uint32_t)bit() << (b & 31);
    return x;
  }
};

bool below_modulus(const u256& x) {
  u256 d;
  return u256_sub(d, x, Fr::modulus()) != 0;
}

int host_poseidon_constants(uint32_t t, uint32_t r_f, uint32_t r_p, int layout, void* ark_out, void* mds_out) {
  if (poseidon_constants_check(t, r_f, r_p, layout, ark_out, mds_out)) return MSM_AMD_INPUT_ERROR;
  PoseidonGrain g(t, r_f, r_p);
  for (uint32_t k = 0; k < (r_f + r_p) * t;) {
    const u256 x = g.integer();
    if (below_modulus(x)) host_put(layout, (uint8_t*)ark_out, k++, Fr::to_mont(x));
  }
  u256 xy[2 * kPoseidonMaxT];
  for (bool again = true; again;) {
    for (uint32_t k = 0; k < 2 * t; ++k) xy[k] = Fr::to_mont(Fr::reduce_once(g.integer()));   // 2^254 < 2 r
    again = false;
    for (uint32_t a = 0; a < 2 * t; ++a)
      for (uint32_t b = a + 1; b < 2 * t; ++b) again |= u256_eq(xy[a], xy[b]);
    // (the paper's script also draws again when some x_i + y_j is zero)
    for (uint32_t i = 0; i < t; ++i)
      for (uint32_t j = 0; j < t; ++j) again |= u256_is_zero(Fr::add(xy[i], xy[t + j]));
  }
  for (uint32_t i = 0; i < t; ++i)
    for (uint32_t j = 0; j < t; ++j) host_put(layout, (uint8_t*)mds_out, i * t + j, ntt_fr_inv(Fr::add(xy[i], xy[t + j])));
  return MSM_AMD_OK;
}

struct PoseidonHostImage {
  const u256* p;
  u256 record(uint32_t i) const { return p[i]; }
};
struct PoseidonHostShape {
  uint32_t t, r_f, r_p;
  int layout;
  std::vector<u256> image;
  u256 tag;
};

// a range of at least 16 permutations per thread, so that a short call starts none
unsigned poseidon_workers(int threads, uint64_t n) { return worker_count(threads, (size_t)((n + 15) >> 4)); }

template <int T, int KIND>
void host_poseidon_run(const PoseidonHostShape& c, const uint8_t* in, uint64_t n, int threads, uint8_t* out) {
  constexpr int IN = KIND == kPoseidonHash ? T - 1 : T, FIRST = T - IN;
  const PoseidonHostImage image{c.image.data()};
  for_ranges(poseidon_workers(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      u256 s[T];
      s[0] = c.tag;
      for (int j = 0; j < IN; ++j) s[FIRST + j] = host_get(c.layout, in, i * IN + j);
      poseidon_permute<T>(s, image, c.r_f, c.r_p);
      if (KIND == kPoseidonHash) host_put(c.layout, out, i, s[0]);
      else
        for (int j = 0; j < T; ++j) host_put(c.layout, out, i * T + j, s[j]);
    }
  });
}

template <int KIND>
void host_poseidon_kind(const PoseidonHostShape& c, const void* in, uint64_t n, int threads, void* out) {
  const uint8_t* src = (const uint8_t*)in;
  uint8_t* dst = (uint8_t*)out;
  if (c.t == 2) host_poseidon_run<2, KIND>(c, src, n, threads, dst);
  else if (c.t == 3) host_poseidon_run<3, KIND>(c, src, n, threads, dst);
  else if (c.t == 4) host_poseidon_run<4, KIND>(c, src, n, threads, dst);
  else host_poseidon_run<5, KIND>(c, src, n, threads, dst);
}

// the shape of a twin's call; false: an argument is wrong
bool host_poseidon_shape(uint32_t t, uint32_t r_f, uint32_t r_p, int layout, const void* ark, const void* mds, const void* tag32,
                         PoseidonHostShape* c) {
  if (poseidon_constants_check(t, r_f, r_p, layout, ark, mds)) return false;
  c->t = t, c->r_f = r_f, c->r_p = r_p, c->layout = layout;
  poseidon_build_image(t, r_f, r_p, layout, ark, mds, &c->image);
  c->tag = tag32 ? fr_read_record(layout, tag32) : u256_zero();
  return true;
}

int host_poseidon_call(int kind, uint32_t t, uint32_t r_f, uint32_t r_p, int layout, const void* ark, const void* mds,
                       const void* tag32, const void* in, size_t n, int threads, void* out) {
  PoseidonHostShape c;
  if (!host_poseidon_shape(t, r_f, r_p, layout, ark, mds, tag32, &c)) return MSM_AMD_INPUT_ERROR;
  if (poseidon_call_check(kind, t, layout, in, n, out, false)) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  if (kind == kPoseidonHash) host_poseidon_kind<kPoseidonHash>(c, in, n, threads, out);
  else host_poseidon_kind<kPoseidonPermute>(c, in, n, threads, out);
  return MSM_AMD_OK;
}

int host_poseidon_merkle_build(uint32_t t, uint32_t r_f, uint32_t r_p, int layout, const void* ark, const void* mds,
                               const void* tag32, const void* leaves, size_t n_leaves, int threads, void* tree, void* root32) {
  PoseidonHostShape c;
  if (!host_poseidon_shape(t, r_f, r_p, layout, ark, mds, tag32, &c)) return MSM_AMD_INPUT_ERROR;
  if (poseidon_merkle_check(t, layout, leaves, n_leaves, tree, false)) return MSM_AMD_INPUT_ERROR;
  const PoseidonTreePlan plan = poseidon_tree_plan(n_leaves, t - 1, 0);
  const uint8_t* src = (const uint8_t*)leaves;
  for (uint32_t k = 0; k < plan.depth; ++k) {
    uint8_t* dst = (uint8_t*)tree + plan.offset[k] * 32;
    host_poseidon_kind<kPoseidonHash>(c, src, plan.count[k], threads, dst);
    src = dst;
  }
  if (root32) std::memcpy(root32, (const uint8_t*)tree + (plan.nodes - 1) * 32, 32);
  return MSM_AMD_OK;
}

int host_poseidon_merkle_paths(uint32_t t, int layout, const void* leaves, size_t n_leaves, const void* tree, const uint64_t* idx,
                               size_t n_idx, int threads, void* out) {
  if (t < kPoseidonMinT || t > kPoseidonMaxT) return MSM_AMD_INPUT_ERROR;
  if (poseidon_paths_check(t, layout, leaves, n_leaves, tree, idx, n_idx, out, false)) return MSM_AMD_INPUT_ERROR;
  if (n_idx == 0) return MSM_AMD_OK;
  const uint32_t arity = t - 1;
  const PoseidonTreePlan plan = poseidon_tree_plan(n_leaves, arity, 0);
  const uint64_t per = (uint64_t)plan.depth * (arity - 1);
  for_ranges(worker_count(threads, (n_idx + 63) >> 6), n_idx, [&](unsigned, size_t lo, size_t hi) {
    for (size_t q = lo; q < hi; ++q) {
      uint64_t pos = idx[q], at = q * per;
      for (uint32_t level = 0; level < plan.depth; ++level, pos /= arity) {
        const uint8_t* src = level == 0 ? (const uint8_t*)leaves : (const uint8_t*)tree + plan.offset[level - 1] * 32;
        for (uint32_t child = 0; child < arity; ++child)
          if (child != pos % arity) host_put(layout, (uint8_t*)out, at++, host_get(layout, src, pos - pos % arity + child));
      }
    }
  });
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

int msm_amd_poseidon_constants(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, void* ark_out, void* mds_out) {
  return msm_amd::host_poseidon_constants(t, r_f, r_p, scalar_layout, ark_out, mds_out);
}

int msm_amd_host_poseidon_permute(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                                  const void* in, size_t n, int threads, void* out) {
  return msm_amd::host_poseidon_call(msm_amd::kPoseidonPermute, t, r_f, r_p, scalar_layout, ark, mds, nullptr, in, n, threads, out);
}

int msm_amd_host_poseidon_hash(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                               const void* tag32, const void* in, size_t n, int threads, void* out) {
  return msm_amd::host_poseidon_call(msm_amd::kPoseidonHash, t, r_f, r_p, scalar_layout, ark, mds, tag32, in, n, threads, out);
}

int msm_amd_host_poseidon_merkle_build(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                                       const void* tag32, const void* leaves, size_t n_leaves, int threads, void* tree,
                                       void* root32) {
  return msm_amd::host_poseidon_merkle_build(t, r_f, r_p, scalar_layout, ark, mds, tag32, leaves, n_leaves, threads, tree, root32);
}

int msm_amd_host_poseidon_merkle_paths(uint32_t t, int scalar_layout, const void* leaves, size_t n_leaves, const void* tree,
                                       const uint64_t* idx, size_t n_idx, int threads, void* out) {
  return msm_amd::host_poseidon_merkle_paths(t, scalar_layout, leaves, n_leaves, tree, idx, n_idx, threads, out);
}

int msm_amd_test_poseidon_plan(uint32_t t, size_t n_leaves, uint32_t top_log, uint64_t counts[40]) {
  using namespace msm_amd;
  if (!counts || t < 3 || t > kPoseidonMaxT || top_log > kPoseidonMaxTopLog || ((uint64_t)n_leaves >> 32) ||
      !poseidon_tree_depth(n_leaves, t - 1))
    return MSM_AMD_INPUT_ERROR;
  const PoseidonTreePlan p = poseidon_tree_plan(n_leaves, t - 1, top_log);
  uint64_t c[40] = {p.launches, p.depth, p.nodes, p.tail_levels, p.tail_nodes, 0, 0, 0};
  for (uint32_t k = 0; k + 1 < p.launches; ++k) c[8 + k] = p.count[k];
  c[8 + p.launches - 1] = p.tail_nodes;
  std::memcpy(counts, c, sizeof c);
  return MSM_AMD_OK;
}

}  // extern "C"
