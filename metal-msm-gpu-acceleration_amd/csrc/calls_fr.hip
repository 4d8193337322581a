// The blocking vector calls over Fr (device_call.h): map, prefix product, batch inversion, polynomials, linear
// combinations, sparse matrices, multilinear tables and sumcheck rounds, gate polynomials, the width scan, Poseidon.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "device_call.h"

// ---- vectors over Fr (msm_amd_fr_map*, msm_amd_fr_batch_inverse*, msm_amd_fr_prefix_product*, msm_amd_fr_poly_*,
// msm_amd_fr_lincomb*) ------------------------------------------------------------------------------------------------------
// Through device_call: the host forms compute over the staged copy of their first operand.  The inversion has two spans
// of kernels: T and the zero count come back as the call's 64-byte record, the host inverts T.  The polynomial calls
// read p_v(z) back through the call's page-locked values buffer, in the one bounded wait behind their kernels.
namespace {

int fr_map_call(msm_amd_ctx* ctx, bool host, int op, int scalar_layout, const void* k32, const void* a, const void* b,
                const void* c, size_t n, void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_map" : "msm_amd_fr_map_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_map_check(op, scalar_layout, k32, a, b, c, n, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const unsigned reads = fr_op_reads(op);
  const void* operand[3] = {a, b, c};
  d.host = d.in_place = host, d.host_in = host ? reads : 0u, d.kernel_ms = kernel_ms;
  for (int i = 0; i < 3; ++i) d.in[i] = operand[i], d.in_bytes[i] = (reads >> i & 1) ? n * 32 : 0;
  d.out = out, d.out_bytes = n * 32;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_fr_map(st, op, scalar_layout, fr_read_k(op, scalar_layout, k32), io.in[0], io.in[1], io.in[2], n, io.out);
    return MSM_AMD_OK;
  });
}

int fr_shift_call(msm_amd_ctx* ctx, bool host, int scalar_layout, const void* k32, const void* a, size_t n, void* out,
                  float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_shift" : "msm_amd_fr_shift_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_shift_check(scalar_layout, k32, a, n, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = a, d.in_bytes[0] = n * 32;
  d.out = out, d.out_bytes = n * 32;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_fr_shift(st, scalar_layout, fr_read_record(scalar_layout, k32), io.in[0], n, io.out);
    return MSM_AMD_OK;
  });
}

// msm_amd_fr_prefix_product* and (sum) msm_amd_fr_prefix_sum*
int fr_prefix_call(msm_amd_ctx* ctx, bool host, bool sum, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec,
                   void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = std::string(sum ? "msm_amd_fr_prefix_sum" : "msm_amd_fr_prefix_product") + (host ? "" : "_device");
  if (kernel_ms) *kernel_ms = 0.f;
  if (!fr_mode_known(mode))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": mode must be MSM_AMD_FR_PREFIX_INCLUSIVE or MSM_AMD_FR_PREFIX_EXCLUSIVE");
  if (const char* why = fr_unary_check(scalar_layout, in, n, n_vec, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrScanLaunch c{};
  c.n = n, c.n_vec = n_vec, c.tile_log = ctx->fr_tile_log, c.layout = scalar_layout, c.mode = mode, c.sum = sum;
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = n * n_vec * 32;
  d.out = out, d.out_bytes = n * n_vec * 32;
  d.work[0] = {&s.work, std::max<size_t>(32, fr_scan_plan(n, n_vec, c.tile_log).records * 32)};
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    c.in = io.in[0], c.out = io.out, c.work = s.work.p;
    launch_fr_scan(st, c);
    return MSM_AMD_OK;
  });
}

int fr_inverse_call(msm_amd_ctx* ctx, bool host, int scalar_layout, const void* in, size_t n, void* out, uint64_t* n_zero,
                    float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_batch_inverse" : "msm_amd_fr_batch_inverse_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_zero) *n_zero = 0;
  if (const char* why = fr_unary_check(scalar_layout, in, n, 1, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  const uint32_t tile_log = ctx->fr_tile_log;
  const FrInvPlan plan = fr_inv_plan(n, tile_log);
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = n * 32;
  d.out = out, d.out_bytes = n * 32;
  d.work[0] = {&s.work, plan.records * 32};
  uint64_t zeros = 0;
  u256 t_inv;
  const int rc = device_call(
      ctx, d,
      [&](hipStream_t st, CallIo& io) {   // span 1: the products; T and the zero count come back
        launch_fr_inv_products(st, scalar_layout, io.in[0], n, tile_log, s.work.p);
        io.record = fr_inv_tail(s.work.p, plan);
        return MSM_AMD_OK;
      },
      [&](const uint8_t* tail, float) {
        u256 total;
        std::memcpy(total.v, tail, 32);
        std::memcpy(&zeros, tail + 32, 8);
        t_inv = ntt_fr_inv(total);   // zeros were read as one: T != 0
      },
      [&](hipStream_t st, const CallIo& io) {   // span 2: every record's inverse
        launch_fr_inv_apply(st, scalar_layout, io.in[0], n, tile_log, s.work.p, t_inv, io.out);
        return MSM_AMD_OK;
      });
  if (rc == MSM_AMD_OK && n_zero) *n_zero = zeros;
  return rc;
}

// p_v(z) come back as raw records through CallState::h_values and leave in the caller's layout
void fr_values_out(const CallState& s, int scalar_layout, size_t n_vec, void* out) {
  for (size_t v = 0; v < n_vec; ++v) {
    u256 x;
    std::memcpy(x.v, s.h_values + v * 32, 32);
    uint32_t rec[8];
    ntt_store(scalar_layout, x, rec);
    std::memcpy((uint8_t*)out + v * 32, rec, 32);
  }
}

// msm_amd_fr_poly_eval* (divide false: out is unused, values required) and msm_amd_fr_poly_div_linear*
int fr_poly_call(msm_amd_ctx* ctx, bool host, bool divide, int scalar_layout, const void* z32, const void* in, size_t n,
                 size_t n_vec, void* out, void* values, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = std::string(divide ? "msm_amd_fr_poly_div_linear" : "msm_amd_fr_poly_eval") + (host ? "" : "_device");
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_poly_check(scalar_layout, z32, in, n, n_vec, out, values, divide, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrPolyLaunch c{};
  c.n = n, c.n_vec = n_vec, c.tile_log = ctx->fr_tile_log, c.layout = scalar_layout, c.divide = divide;
  c.z = fr_read_record(scalar_layout, z32);
  const FrScanPlan plan = fr_scan_plan(n, n_vec, c.tile_log);
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = n * n_vec * 32;
  d.out = out, d.out_bytes = divide ? n * n_vec * 32 : 0;
  d.work[0] = {&s.work, fr_poly_values(plan) + n_vec * 32};
  d.values_bytes = values ? n_vec * 32 : 0;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
    c.in = io.in[0], c.out = io.out, c.work = s.work.p;
    launch_fr_poly(st, c);
    io.values = (const uint8_t*)s.work.p + fr_poly_values(plan);
    return MSM_AMD_OK;
  });
  if (rc == MSM_AMD_OK && values) fr_values_out(s, scalar_layout, n_vec, values);
  return rc;
}

// msm_amd_fr_poly_eval_points (divide false: out is unused, values required) and msm_amd_fr_poly_div_points: the launches
// of one point at k points (launch_fr_poly_points), the workspace k times that of fr_poly_call.  The k n_vec values come
// back point-major and leave as values[v k + j].
int fr_poly_points_call(msm_amd_ctx* ctx, int mem, bool divide, int scalar_layout, const void* z, size_t k, const void* in,
                        size_t n, size_t n_vec, void* out, void* values, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = divide ? "msm_amd_fr_poly_div_points" : "msm_amd_fr_poly_eval_points";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_poly_points_check(mem, scalar_layout, z, k, in, n, n_vec, out, values, divide))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const bool host = mem == MSM_AMD_MEM_HOST;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrPolyPointsLaunch c{};
  c.n = n, c.n_vec = n_vec, c.tile_log = ctx->fr_tile_log, c.layout = scalar_layout, c.divide = divide, c.k = (uint32_t)k;
  for (size_t j = 0; j < k; ++j) c.z[j] = fr_read_record(scalar_layout, (const uint8_t*)z + j * 32);
  const FrScanPlan plan = fr_scan_plan(n, n_vec, c.tile_log);
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = n * n_vec * 32;
  d.out = out, d.out_bytes = divide ? n * n_vec * 32 : 0;
  d.work[0] = {&s.work, (size_t)fr_poly_points_records(plan, n_vec, k) * 32};
  d.values_bytes = values ? k * n_vec * 32 : 0;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
    c.in = io.in[0], c.out = io.out, c.work = s.work.p;
    launch_fr_poly_points(st, c);
    io.values = (const uint8_t*)s.work.p + fr_poly_points_values(plan, k);
    return MSM_AMD_OK;
  });
  if (rc != MSM_AMD_OK || !values) return rc;
  for (size_t j = 0; j < k; ++j)
    for (size_t v = 0; v < n_vec; ++v) {
      u256 x;
      std::memcpy(x.v, s.h_values + (j * n_vec + v) * 32, 32);
      uint32_t rec[8];
      ntt_store(scalar_layout, x, rec);
      std::memcpy((uint8_t*)values + (v * k + j) * 32, rec, 32);
    }
  return rc;
}

int fr_lincomb_call(msm_amd_ctx* ctx, bool host, int scalar_layout, const void* k32, const void* a, size_t n, size_t n_vec,
                    void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_lincomb" : "msm_amd_fr_lincomb_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_lincomb_check(scalar_layout, k32, a, n, n_vec, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  // the host form folds into the first vector of the staged copy
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = a, d.in_bytes[0] = n * n_vec * 32;
  d.out = out, d.out_bytes = n * 32;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_fr_lincomb(st, scalar_layout, fr_read_record(scalar_layout, k32), io.in[0], n, n_vec, io.out);
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_fr_poly_eval(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* coeffs, size_t n, size_t n_vec,
                         void* y_out) {
  return fr_poly_call(ctx, true, false, scalar_layout, z32, coeffs, n, n_vec, nullptr, y_out, nullptr);
}

int msm_amd_fr_poly_eval_device(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* d_coeffs, size_t n,
                                size_t n_vec, void* y_out, float* kernel_ms) {
  return fr_poly_call(ctx, false, false, scalar_layout, z32, d_coeffs, n, n_vec, nullptr, y_out, kernel_ms);
}

int msm_amd_fr_poly_div_linear(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* in, size_t n, size_t n_vec,
                               void* out, void* rem_out) {
  return fr_poly_call(ctx, true, true, scalar_layout, z32, in, n, n_vec, out, rem_out, nullptr);
}

int msm_amd_fr_poly_div_linear_device(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* d_in, size_t n,
                                      size_t n_vec, void* d_out, void* rem_out, float* kernel_ms) {
  return fr_poly_call(ctx, false, true, scalar_layout, z32, d_in, n, n_vec, d_out, rem_out, kernel_ms);
}

int msm_amd_fr_poly_eval_points(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* z, size_t k, const void* coeffs,
                                size_t n, size_t n_vec, void* y_out, float* kernel_ms) {
  return fr_poly_points_call(ctx, mem, false, scalar_layout, z, k, coeffs, n, n_vec, nullptr, y_out, kernel_ms);
}

int msm_amd_fr_poly_div_points(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* z, size_t k, const void* in, size_t n,
                               size_t n_vec, void* out, void* vals_out, float* kernel_ms) {
  return fr_poly_points_call(ctx, mem, true, scalar_layout, z, k, in, n, n_vec, out, vals_out, kernel_ms);
}

int msm_amd_fr_lincomb(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* a, size_t n, size_t n_vec, void* out) {
  return fr_lincomb_call(ctx, true, scalar_layout, k32, a, n, n_vec, out, nullptr);
}

int msm_amd_fr_lincomb_device(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* d_a, size_t n, size_t n_vec,
                              void* d_out, float* kernel_ms) {
  return fr_lincomb_call(ctx, false, scalar_layout, k32, d_a, n, n_vec, d_out, kernel_ms);
}

int msm_amd_fr_map(msm_amd_ctx* ctx, int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c,
                   size_t n, void* out) {
  return fr_map_call(ctx, true, op, scalar_layout, k32, a, b, c, n, out, nullptr);
}

int msm_amd_fr_map_device(msm_amd_ctx* ctx, int op, int scalar_layout, const void* k32, const void* d_a, const void* d_b,
                          const void* d_c, size_t n, void* d_out, float* kernel_ms) {
  return fr_map_call(ctx, false, op, scalar_layout, k32, d_a, d_b, d_c, n, d_out, kernel_ms);
}

int msm_amd_fr_batch_inverse(msm_amd_ctx* ctx, int scalar_layout, const void* in, size_t n, void* out, uint64_t* n_zero) {
  return fr_inverse_call(ctx, true, scalar_layout, in, n, out, n_zero, nullptr);
}

int msm_amd_fr_batch_inverse_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_in, size_t n, void* d_out,
                                    uint64_t* n_zero, float* kernel_ms) {
  return fr_inverse_call(ctx, false, scalar_layout, d_in, n, d_out, n_zero, kernel_ms);
}

int msm_amd_fr_prefix_product(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec,
                              void* out) {
  return fr_prefix_call(ctx, true, false, scalar_layout, mode, in, n, n_vec, out, nullptr);
}

int msm_amd_fr_prefix_product_device(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* d_in, size_t n, size_t n_vec,
                                     void* d_out, float* kernel_ms) {
  return fr_prefix_call(ctx, false, false, scalar_layout, mode, d_in, n, n_vec, d_out, kernel_ms);
}

int msm_amd_fr_prefix_sum(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, void* out) {
  return fr_prefix_call(ctx, true, true, scalar_layout, mode, in, n, n_vec, out, nullptr);
}

int msm_amd_fr_prefix_sum_device(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* d_in, size_t n, size_t n_vec,
                                 void* d_out, float* kernel_ms) {
  return fr_prefix_call(ctx, false, true, scalar_layout, mode, d_in, n, n_vec, d_out, kernel_ms);
}

int msm_amd_fr_shift(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* a, size_t n, void* out) {
  return fr_shift_call(ctx, true, scalar_layout, k32, a, n, out, nullptr);
}

int msm_amd_fr_shift_device(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* d_a, size_t n, void* d_out,
                            float* kernel_ms) {
  return fr_shift_call(ctx, false, scalar_layout, k32, d_a, n, d_out, kernel_ms);
}

}  // extern "C"

// ---- lookup tables over Fr (msm_amd_fr_lookup_*) ------------------------------------------------------------------------------
// A handle is validated by membership in ctx->live_fr_lookup, under the lock.  The build has one bounded wait (that of
// handle_build_tail): the statistics of the index come back with it through the page-locked record of CallState.  A
// multiplicities call is a device_call whose 64-byte record is the report: the counters and the report live in
// CallState::work, the finish kernel reads the miss counter on the device, and the device form is done after the one wait
// for its record.  The host form stages m in CallState::out and the row indices behind the report, and copies them back
// in a second span -- m only if the call does not fail for a miss, so that the caller's m_out stays untouched then.
namespace {

const char* const kNotLookup = ": not a lookup table handle of this ctx";

int fr_lookup_build_call(msm_amd_ctx* ctx, bool host, int scalar_layout, const void* table, size_t n_rows,
                         msm_amd_fr_lookup** out, float* kernel_ms) {
  const std::string who = host ? "msm_amd_fr_lookup_build" : "msm_amd_fr_lookup_build_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (!ctx || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": null pointer");
  *out = nullptr;
  if (const char* why = fr_lookup_table_check(scalar_layout, table, n_rows, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": " + why);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  const FrLookupPlan plan = fr_lookup_plan(n_rows, fr_lookup_hash_bits_knob());
  CallState& s = ctx->calls;
  if (!s.h_record) HIP_TRY(ctx, hipHostMalloc((void**)&s.h_record, sizeof(PointCounters), hipHostMallocDefault));
  if (kernel_ms)
    for (int k = 0; k < 2; ++k)
      if (!s.ev[k]) HIP_TRY(ctx, hipEventCreate(&s.ev[k]));
  std::vector<u256> rows;   // host form: the residues are formed here and uploaded into the image
  if (host) {
    rows.resize(n_rows);
    for (size_t j = 0; j < n_rows; ++j) rows[j] = fr_read_record(scalar_layout, (const uint8_t*)table + j * 32);
  }
  int up = MSM_AMD_OK;
  hipError_t tail = hipSuccess;
  if (int rc = handle_build_tail(
          ctx, ctx->live_fr_lookup, plan.bytes, "a lookup table", "lookup table build",
          [&](void* d_mem) {
            hipStream_t st = ctx->stream;
            if (host && (up = staged_upload(ctx, (uint8_t*)d_mem + plan.rows_off, rows.data(), n_rows * 32, st))) return;
            if (kernel_ms) tail = hipEventRecord(s.ev[0], st);
            launch_fr_lookup_build(st, plan, n_rows, scalar_layout, host ? nullptr : table, d_mem);
            if (kernel_ms && tail == hipSuccess) tail = hipEventRecord(s.ev[1], st);
            if (tail == hipSuccess)
              tail = hipMemcpyAsync(s.h_record, (const uint8_t*)d_mem + plan.stats_off, kLookupStatWords * 4,
                                    hipMemcpyDeviceToHost, st);
          },
          out))
    return rc;
  msm_amd_fr_lookup* h = *out;
  uint32_t stats[kLookupStatWords];
  std::memcpy(stats, s.h_record, sizeof stats);
  std::string why;
  if (up) why = ctx->last_error;
  else if (tail != hipSuccess) why = hipGetErrorString(tail), up = MSM_AMD_PIPELINE_ERROR;
  else if (stats[kLookupError]) why = "an insert ran through every slot of the index", up = MSM_AMD_PIPELINE_ERROR;
  if (up) {   // nothing may read the allocation
    *out = nullptr;
    handle_free(ctx, ctx->live_fr_lookup, h, "");
    return fail(ctx, up, who + ": " + why);
  }
  if (kernel_ms) *kernel_ms = event_span(s.ev[0], s.ev[1]);
  h->n_rows = n_rows, h->n_distinct = stats[kLookupDistinct], h->longest_probe = stats[kLookupLongest], h->plan = plan;
  return MSM_AMD_OK;
}

// msm_amd_fr_lookup_build_sorted: the table is sorted by the kernels of msm_amd_fr_sort straight into the rows of the new
// image -- the keys and the digit mask, one bounded wait for the mask, the passes, and a final gather that writes reduced
// Montgomery residues -- then the insert pass of a plain build indexes the sorted rows.  The keys and the wait for the mask
// come before the image is allocated; the second wait is that of handle_build_tail, which also brings the statistics and
// (host form) the staged permutation.
int fr_lookup_build_sorted_call(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* table, size_t n_rows,
                                uint32_t* perm_out, msm_amd_fr_lookup** out, float* kernel_ms) {
  const std::string who = "msm_amd_fr_lookup_build_sorted";
  if (kernel_ms) *kernel_ms = 0.f;
  if (!ctx || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": null pointer");
  *out = nullptr;
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE)
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE");
  const bool host = mem == MSM_AMD_MEM_HOST;
  if (const char* why = fr_lookup_table_check(scalar_layout, table, n_rows, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": " + why);
  if (!host && ((uintptr_t)perm_out & 3u)) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": device perm_out must be 4-byte aligned");
  if (perm_out && (uintptr_t)perm_out < (uintptr_t)table + n_rows * 32 && (uintptr_t)table < (uintptr_t)perm_out + n_rows * 4)
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": perm_out must not overlap the table");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  if (!drain_or_mark_stalled(ctx))
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, who + ": device busy past the wait bound of " + std::to_string(ctx->wait_timeout_ms) + " ms");
  const FrLookupPlan plan = fr_lookup_plan(n_rows, fr_lookup_hash_bits_knob());
  CallState& s = ctx->calls;
  FrSortLaunch c{};
  c.n = n_rows, c.n_vec = 1, c.layout = scalar_layout;
  c.plan = fr_sort_plan(n_rows, 1, 0);
  const size_t perm_at = (size_t)((c.plan.bytes + 15) & ~(uint64_t)15);   // host form: the staged permutation
  // the ctx is idle: every buffer is sized before anything is enqueued
  if (int rc = ensure(ctx, s.work, perm_at + (host && perm_out ? n_rows * 4 : 0))) return rc;
  if (host)
    if (int rc = ensure(ctx, s.in[0], n_rows * 32)) return rc;
  if (!s.h_record) HIP_TRY(ctx, hipHostMalloc((void**)&s.h_record, sizeof(PointCounters), hipHostMallocDefault));
  if (kernel_ms)
    for (hipEvent_t& e : s.ev)
      if (!e) HIP_TRY(ctx, hipEventCreate(&e));
  // span 1, before the image exists: the keys into CallState::work and the digit mask behind a bounded wait of its own, so
  // that handle_build_tail below keeps its contract (its callable only enqueues, the helper waits once)
  hipStream_t st = ctx->stream;
  c.in = table, c.work = s.work.p;
  if (host) {
    if (int rc = staged_upload(ctx, s.in[0].p, table, n_rows * 32, st)) return rc;
    c.in = s.in[0].p;
  }
  if (kernel_ms) HIP_TRY(ctx, hipEventRecord(s.ev[0], st));
  launch_fr_sort_keys(st, c);
  HIP_TRY(ctx, hipGetLastError());
  if (kernel_ms) HIP_TRY(ctx, hipEventRecord(s.ev[1], st));
  HIP_TRY(ctx, hipMemcpyAsync(s.h_record, s.work.p, kSortRecordBytes, hipMemcpyDeviceToHost, st));
  if (int rc = sync_stream_bounded(ctx, st, who.c_str())) return rc;
  uint32_t mask;
  std::memcpy(&mask, s.h_record, 4);
  // span 2: the passes and the final gather into the rows of the new image, the insert pass, the statistics
  int up = MSM_AMD_OK;
  hipError_t tail = hipSuccess;
  if (int rc = handle_build_tail(
          ctx, ctx->live_fr_lookup, plan.bytes, "a lookup table", "sorted lookup table build",
          [&](void* d_mem) {
            // the rows of the image are reduced Montgomery residues whatever the caller's layout is
            c.layout = MSM_AMD_SCALAR_MONT_LE, c.out = (uint8_t*)d_mem + plan.rows_off;
            c.perm_out = !perm_out ? nullptr : host ? (uint32_t*)((uint8_t*)s.work.p + perm_at) : perm_out;
            if (kernel_ms) tail = hipEventRecord(s.ev[2], st);
            launch_fr_sort_passes(st, c, mask);
            launch_fr_lookup_build(st, plan, n_rows, scalar_layout, nullptr, d_mem);
            if (kernel_ms && tail == hipSuccess) tail = hipEventRecord(s.ev[3], st);
            if (tail == hipSuccess)
              tail = hipMemcpyAsync(s.h_record, (const uint8_t*)d_mem + plan.stats_off, kLookupStatWords * 4,
                                    hipMemcpyDeviceToHost, st);
            if (tail == hipSuccess && host && perm_out)
              tail = hipMemcpyAsync(perm_out, c.perm_out, n_rows * 4, hipMemcpyDeviceToHost, st);
          },
          out))
    return rc;
  msm_amd_fr_lookup* h = *out;
  uint32_t stats[kLookupStatWords];
  std::memcpy(stats, s.h_record, sizeof stats);
  std::string why;
  if (tail != hipSuccess) why = hipGetErrorString(tail), up = MSM_AMD_PIPELINE_ERROR;
  else if (stats[kLookupError]) why = "an insert ran through every slot of the index", up = MSM_AMD_PIPELINE_ERROR;
  if (up) {   // nothing may read the allocation
    *out = nullptr;
    handle_free(ctx, ctx->live_fr_lookup, h, "");
    return fail(ctx, up, who + ": " + why);
  }
  if (kernel_ms) *kernel_ms = event_span(s.ev[0], s.ev[1]) + event_span(s.ev[2], s.ev[3]);
  h->n_rows = n_rows, h->n_distinct = stats[kLookupDistinct], h->longest_probe = stats[kLookupLongest], h->plan = plan;
  h->sorted = true;
  return MSM_AMD_OK;
}

int fr_lookup_mult_call(msm_amd_ctx* ctx, const msm_amd_fr_lookup* handle, bool host, int scalar_layout, int on_missing,
                        const void* in, size_t n, size_t n_vec, void* m_out, uint32_t* idx_out, uint64_t* report,
                        float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_lookup_multiplicities" : "msm_amd_fr_lookup_multiplicities_device";
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_lookup* t = find_handle(ctx->live_fr_lookup, handle);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + kNotLookup);
  if (const char* why = fr_lookup_call_check(scalar_layout, on_missing, t->n_rows, in, n, n_vec, m_out, idx_out, report, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  const size_t total = n * n_vec;
  if (!host) {
    const uintptr_t lo = (uintptr_t)t->d_mem, hi = lo + t->bytes, a = (uintptr_t)m_out, b = (uintptr_t)idx_out;
    if ((a < hi && lo < a + t->n_rows * 32) || (idx_out && b < hi && lo < b + total * 4))
      return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": d_m_out and d_idx_out must not overlap the table");
  }
  CallState& s = ctx->calls;
  FrLookupLaunch c{};
  c.image = t->d_mem, c.plan = t->plan, c.n_rows = t->n_rows, c.layout = scalar_layout, c.on_missing = on_missing;
  c.count_form = fr_lookup_count_knob(), c.total = total;
  c.at = fr_lookup_work(t->n_rows, host && idx_out ? total : 0);
  d.host_in = host && total ? 1u : 0u, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = total * 32;
  d.work[0] = {&s.work, (size_t)c.at.bytes};
  if (host) d.work[1] = {&s.out, (size_t)t->n_rows * 32};
  uint64_t rep[kLookupReportWords] = {};
  auto launch = [&](hipStream_t st, CallIo& io) {
    uint8_t* work = (uint8_t*)s.work.p;
    c.in = io.in[0], c.work = work, c.m_out = host ? s.out.p : m_out;
    c.idx_out = !idx_out || !total ? nullptr : host ? (uint32_t*)(work + c.at.idx_off) : idx_out;
    launch_fr_lookup_multiplicities(st, c);
    io.record = work + c.at.report_off;
    return MSM_AMD_OK;
  };
  auto then = [&](const uint8_t* record, float) { std::memcpy(rep, record, sizeof rep); };
  auto strict_miss = [&] { return on_missing == kLookupStrict && total && rep[kLookupMissing] != 0; };
  int rc;
  if (host)
    rc = device_call(ctx, d, launch, then, [&](hipStream_t st, const CallIo&) -> int {
      const uint8_t* work = (const uint8_t*)s.work.p;
      if (c.idx_out) HIP_TRY(ctx, hipMemcpyAsync(idx_out, work + c.at.idx_off, total * 4, hipMemcpyDeviceToHost, st));
      if (!strict_miss() && !rep[kLookupReportError])
        HIP_TRY(ctx, hipMemcpyAsync(m_out, s.out.p, t->n_rows * 32, hipMemcpyDeviceToHost, st));
      return MSM_AMD_OK;
    });
  else
    rc = device_call(ctx, d, launch, then);
  if (rc) return rc;
  if (rep[kLookupReportError])
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, d.who + ": a probe ran through every slot of the index");
  for (int k = 0; k < 4; ++k) report[k] = total ? rep[k] : 0;
  if (strict_miss())
    return fail(ctx, MSM_AMD_INPUT_ERROR,
                d.who + ": " + std::to_string(rep[kLookupMissing]) + " of " + std::to_string(total) +
                    " inputs are not in the table, the first at flat index " + std::to_string(rep[kLookupFirstMissing]) +
                    " (MSM_AMD_LOOKUP_STRICT; m_out is untouched)");
  return MSM_AMD_OK;
}

// msm_amd_fr_lookup_permute and msm_amd_fr_lookup_permute_as: one span of kernels, the report as the call's record.  Host form:
// the outputs asked for are staged one behind the other in CallState::out and copied back in a second span, only if nothing
// was missing.  Device form: the fill kernel writes the caller's buffers, and writes nothing if anything was missing; the call
// is done after the one wait for its record.
int fr_lookup_permute_call(msm_amd_ctx* ctx, const char* who, const msm_amd_fr_lookup* handle, int mem, int scalar_layout,
                           int arrangement, const void* in, size_t n, size_t n_vec, void* a_out, void* s_out, uint64_t* report,
                           float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = who;
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_lookup* t = find_handle(ctx->live_fr_lookup, handle);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + kNotLookup);
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE)
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE");
  if (arrangement != kPermuteRows && arrangement != kPermuteHalo2)
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": arrangement must be MSM_AMD_PERMUTE_ROWS or MSM_AMD_PERMUTE_HALO2");
  if (arrangement == kPermuteHalo2 && !t->sorted)
    return fail(ctx, MSM_AMD_INPUT_ERROR,
                d.who + ": MSM_AMD_PERMUTE_HALO2 needs a handle of msm_amd_fr_lookup_build_sorted (the rows in value order)");
  const bool host = mem == MSM_AMD_MEM_HOST;
  if (const char* why = fr_permute_call_check(scalar_layout, t->n_rows, in, n, n_vec, a_out, s_out, report))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  const size_t total = n * n_vec, bytes = total * 32;
  if (!host && total) {
    if (((uintptr_t)in | (uintptr_t)a_out | (uintptr_t)s_out) & 15u)
      return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": device records must be 16-byte aligned");
    const uintptr_t lo = (uintptr_t)t->d_mem, hi = lo + t->bytes;
    for (const void* p : {in, (const void*)a_out, (const void*)s_out})
      if (p && (uintptr_t)p < hi && lo < (uintptr_t)p + bytes)
        return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": in, a_out and s_out must not overlap the table");
  }
  for (int k = 0; k < 4; ++k) report[k] = 0;
  if (total == 0) return MSM_AMD_OK;
  CallState& s = ctx->calls;
  FrPermuteLaunch c{};
  c.probe.image = t->d_mem, c.probe.plan = t->plan, c.probe.n_rows = t->n_rows, c.probe.layout = scalar_layout;
  c.probe.count_form = fr_lookup_count_knob(), c.probe.total = total;
  c.tile_log = fr_permute_tile_log_knob(), c.n = n, c.n_vec = n_vec;
  c.fill_form = fr_permute_fill_knob(), c.arrangement = arrangement;
  c.plan = fr_permute_plan(t->n_rows, n_vec, c.tile_log);
  d.host_in = host ? 1u : 0u, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = bytes;
  d.work[0] = {&s.work, (size_t)(c.fill_form == kPermuteFillScan ? fr_permute_owner_plan(c.plan, n, n_vec, c.tile_log).bytes
                                                                 : c.plan.bytes)};
  const size_t s_at = a_out ? bytes : 0;   // S' lies behind A' if both are asked for
  if (host) d.work[1] = {&s.out, s_at + (s_out ? bytes : 0)};
  uint64_t rep[kLookupReportWords] = {};
  auto staged = [&] { return (uint8_t*)s.out.p; };
  auto launch = [&](hipStream_t st, CallIo& io) {
    c.probe.in = io.in[0], c.work = s.work.p;
    c.a_out = !a_out ? nullptr : host ? staged() : a_out;
    c.s_out = !s_out ? nullptr : host ? staged() + s_at : s_out;
    launch_fr_lookup_permute(st, c);
    io.record = (const uint8_t*)s.work.p + c.plan.report_off;
    return MSM_AMD_OK;
  };
  auto then = [&](const uint8_t* record, float) { std::memcpy(rep, record, sizeof rep); };
  int rc;
  if (host)
    rc = device_call(ctx, d, launch, then, [&](hipStream_t st, const CallIo&) -> int {
      if (rep[kLookupMissing] || rep[kLookupReportError]) return MSM_AMD_OK;
      if (a_out) HIP_TRY(ctx, hipMemcpyAsync(a_out, staged(), bytes, hipMemcpyDeviceToHost, st));
      if (s_out) HIP_TRY(ctx, hipMemcpyAsync(s_out, staged() + s_at, bytes, hipMemcpyDeviceToHost, st));
      return MSM_AMD_OK;
    });
  else
    rc = device_call(ctx, d, launch, then);
  if (rc) return rc;
  if (rep[kLookupReportError])
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, d.who + ": a probe ran through every slot of the index");
  for (int k = 0; k < 4; ++k) report[k] = rep[k];
  if (rep[kLookupMissing])
    return fail(ctx, MSM_AMD_INPUT_ERROR,
                d.who + ": " + std::to_string(rep[kLookupMissing]) + " of " + std::to_string(total) +
                    " inputs are not in the table, the first at flat index " + std::to_string(rep[kLookupFirstMissing]) +
                    " (a_out and s_out are untouched)");
  return MSM_AMD_OK;
}

}  // namespace

extern "C" {

int msm_amd_fr_lookup_permute(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout, const void* in, size_t n,
                              size_t n_vec, void* a_out, void* s_out, uint64_t report[4]) {
  return fr_lookup_permute_call(ctx, "msm_amd_fr_lookup_permute", lookup, MSM_AMD_MEM_HOST, scalar_layout, kPermuteRows, in, n,
                                n_vec, a_out, s_out, report, nullptr);
}

int msm_amd_fr_lookup_permute_as(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int mem, int scalar_layout, int arrangement,
                                 const void* in, size_t n, size_t n_vec, void* a_out, void* s_out, uint64_t report[4],
                                 float* kernel_ms) {
  return fr_lookup_permute_call(ctx, "msm_amd_fr_lookup_permute_as", lookup, mem, scalar_layout, arrangement, in, n, n_vec,
                                a_out, s_out, report, kernel_ms);
}

int msm_amd_fr_lookup_sorted(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int* sorted) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_lookup* t = find_handle(ctx->live_fr_lookup, lookup);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_fr_lookup_sorted") + kNotLookup);
  if (!sorted) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_fr_lookup_sorted: null pointer");
  *sorted = t->sorted ? 1 : 0;
  return MSM_AMD_OK;
}

int msm_amd_test_fr_lookup_image(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, void** image) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_lookup* t = find_handle(ctx->live_fr_lookup, lookup);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_test_fr_lookup_image") + kNotLookup);
  if (!image) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_fr_lookup_image: null pointer");
  *image = t->d_mem;
  return MSM_AMD_OK;
}

int msm_amd_fr_lookup_build(msm_amd_ctx* ctx, int scalar_layout, const void* table, size_t n_rows, msm_amd_fr_lookup** out) {
  return fr_lookup_build_call(ctx, true, scalar_layout, table, n_rows, out, nullptr);
}

int msm_amd_fr_lookup_build_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_table, size_t n_rows,
                                   msm_amd_fr_lookup** out, float* kernel_ms) {
  return fr_lookup_build_call(ctx, false, scalar_layout, d_table, n_rows, out, kernel_ms);
}

int msm_amd_fr_lookup_build_sorted(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* table, size_t n_rows,
                                   uint32_t* perm_out, msm_amd_fr_lookup** out, float* kernel_ms) {
  return fr_lookup_build_sorted_call(ctx, mem, scalar_layout, table, n_rows, perm_out, out, kernel_ms);
}

int msm_amd_fr_lookup_info(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, size_t* n_rows, size_t* n_distinct,
                           size_t* capacity, size_t* device_bytes, size_t* longest_probe) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_lookup* t = find_handle(ctx->live_fr_lookup, lookup);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_fr_lookup_info") + kNotLookup);
  if (n_rows) *n_rows = t->n_rows;
  if (n_distinct) *n_distinct = t->n_distinct;
  if (capacity) *capacity = t->plan.capacity;
  if (device_bytes) *device_bytes = t->bytes;
  if (longest_probe) *longest_probe = t->longest_probe;
  return MSM_AMD_OK;
}

int msm_amd_fr_lookup_free(msm_amd_ctx* ctx, msm_amd_fr_lookup* lookup) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return handle_free(ctx, ctx->live_fr_lookup, lookup, "msm_amd_fr_lookup_free: not a lookup table handle of this ctx");
}

int msm_amd_fr_lookup_multiplicities(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout, int on_missing,
                                     const void* in, size_t n, size_t n_vec, void* m_out, uint32_t* idx_out,
                                     uint64_t report[4]) {
  return fr_lookup_mult_call(ctx, lookup, true, scalar_layout, on_missing, in, n, n_vec, m_out, idx_out, report, nullptr);
}

int msm_amd_fr_lookup_multiplicities_device(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout,
                                            int on_missing, const void* d_in, size_t n, size_t n_vec, void* d_m_out,
                                            uint32_t* d_idx_out, uint64_t report[4], float* kernel_ms) {
  return fr_lookup_mult_call(ctx, lookup, false, scalar_layout, on_missing, d_in, n, n_vec, d_m_out, d_idx_out, report,
                             kernel_ms);
}

}  // extern "C"

// ---- sort by canonical value (msm_amd_fr_sort) -------------------------------------------------------------------------------
// A device_call of two spans: the keys and the digit mask, which comes back as the first word of the call's 64-byte record in
// the one bounded wait, then the passes the mask asks for and the final gather.  The keys, the pairs and the histograms live in
// CallState::work.  The host form sorts over the staged copy of its input; its permutation is staged behind the workspace
// and copied back at the end of the second span.
namespace {

int fr_sort_call(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* in, size_t n, size_t n_vec, void* out,
                 uint32_t* perm_out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = "msm_amd_fr_sort";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_sort_call_check(mem, scalar_layout, in, n, n_vec, out, perm_out))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  const size_t total = n * n_vec;
  if (total == 0) return MSM_AMD_OK;
  const bool host = mem == MSM_AMD_MEM_HOST;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrSortLaunch c{};
  c.n = n, c.n_vec = n_vec, c.layout = scalar_layout;
  c.plan = fr_sort_plan(n, n_vec, 0);
  const size_t perm_at = (size_t)((c.plan.bytes + 15) & ~(uint64_t)15);   // host form: the staged permutation
  d.host = d.in_place = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = total * 32;
  d.out = out, d.out_bytes = out ? total * 32 : 0;
  d.work[0] = {&s.work, perm_at + (host && perm_out ? total * 4 : 0)};
  uint32_t mask = 0;
  return device_call(
      ctx, d,
      [&](hipStream_t st, CallIo& io) {
        c.in = io.in[0], c.work = s.work.p;
        launch_fr_sort_keys(st, c);
        io.record = s.work.p;
        return MSM_AMD_OK;
      },
      [&](const uint8_t* record, float) { std::memcpy(&mask, record, 4); },
      [&](hipStream_t st, const CallIo& io) -> int {
        c.out = out ? io.out : nullptr;
        c.perm_out = !perm_out ? nullptr : host ? (uint32_t*)((uint8_t*)s.work.p + perm_at) : perm_out;
        launch_fr_sort_passes(st, c, mask);
        if (host && perm_out) HIP_TRY(ctx, hipMemcpyAsync(perm_out, c.perm_out, total * 4, hipMemcpyDeviceToHost, st));
        return MSM_AMD_OK;
      });
}

}  // namespace

extern "C" {

int msm_amd_fr_sort(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* in, size_t n, size_t n_vec, void* out,
                    uint32_t* perm_out, float* kernel_ms) {
  return fr_sort_call(ctx, mem, scalar_layout, in, n, n_vec, out, perm_out, kernel_ms);
}

}  // extern "C"

// ---- sparse matrix times vector over Fr (msm_amd_fr_matrix_*, msm_amd_fr_matvec*) ------------------------------------------
// The build checks every column on the host before anything is uploaded, so that no index of the image can leave x, the
// dictionary or the partials.  A product is a device_call: x through the staging in the host form, the partial sums of the
// split rows in CallState::work, the launches of launch_fr_matvec on the main stream.
namespace {

int fr_matvec_call(msm_amd_ctx* ctx, const msm_amd_fr_matrix* handle, bool host, int scalar_layout, const void* x, void* y,
                   float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_matvec" : "msm_amd_fr_matvec_device";
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_matrix* m = find_handle(ctx->live_fr_mat, handle);
  if (!m) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": not a matrix handle of this ctx");
  if (const char* why = fr_matvec_check(scalar_layout, m->n_rows, m->n_cols, x, y, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (!host) {
    const uintptr_t lo = (uintptr_t)m->d_mem, hi = lo + m->bytes, a = (uintptr_t)x, b = (uintptr_t)y;
    if ((a < hi && lo < a + m->n_cols * 32) || (b < hi && lo < b + m->n_rows * 32))
      return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": d_x and d_y must not overlap the matrix");
  }
  CallState& s = ctx->calls;
  FrMatLaunch c{};
  c.image = m->d_mem, c.at = m->at, c.plan = m->plan, c.n_rows = m->n_rows, c.long_rows = m->long_rows, c.layout = scalar_layout;
  c.signs = ctx->fr_mat_signs;
  d.host = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = x, d.in_bytes[0] = m->n_cols * 32;
  d.out = y, d.out_bytes = m->n_rows * 32;
  d.work[0] = {&s.work, std::max<size_t>(32, m->plan.partials * 32)};
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    c.x = io.in[0], c.y = io.out, c.work = s.work.p;
    launch_fr_matvec(st, c);
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_fr_matrix_build(msm_amd_ctx* ctx, int scalar_layout, size_t n_rows, size_t n_cols, const uint64_t* row_ptr,
                            const uint32_t* col_idx, const void* values, msm_amd_fr_matrix** out) {
  if (!ctx || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_fr_matrix_build: null pointer");
  *out = nullptr;
  if (const char* why = fr_matrix_check(scalar_layout, n_rows, n_cols, row_ptr, col_idx, values))
    return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_fr_matrix_build: ") + why);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  FrMatPlan plan;
  FrMatImage at;
  uint64_t n_distinct = 0, dict_records = 0;
  std::vector<uint8_t> image;
  fr_mat_build_image(scalar_layout, n_rows, row_ptr, col_idx, values, ctx->fr_mat_long, ctx->fr_mat_seg_log, &plan, &at,
                     &n_distinct, &dict_records, &image);
  int up = MSM_AMD_OK;
  if (int rc = handle_build_tail(ctx, ctx->live_fr_mat, at.bytes, "a sparse matrix", "matrix build",
                                 [&](void* d_mem) { up = staged_upload(ctx, d_mem, image.data(), image.size(), ctx->stream); },
                                 out))
    return rc;
  if (up) {   // the upload did not go through: nothing may read the allocation
    msm_amd_fr_matrix* h = *out;
    *out = nullptr;
    const std::string why = ctx->last_error;
    handle_free(ctx, ctx->live_fr_mat, h, "");
    return fail(ctx, up, "msm_amd_fr_matrix_build: " + why);
  }
  msm_amd_fr_matrix* h = *out;
  h->n_rows = n_rows, h->n_cols = n_cols, h->nnz = row_ptr[n_rows], h->n_distinct = n_distinct;
  h->long_rows = ctx->fr_mat_long, h->plan = plan, h->at = at;
  return MSM_AMD_OK;
}

int msm_amd_fr_matrix_info(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, size_t* n_rows, size_t* n_cols, size_t* nnz,
                           size_t* n_distinct, size_t* device_bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_fr_matrix* m = find_handle(ctx->live_fr_mat, matrix);
  if (!m) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_fr_matrix_info: not a matrix handle of this ctx");
  if (n_rows) *n_rows = m->n_rows;
  if (n_cols) *n_cols = m->n_cols;
  if (nnz) *nnz = m->nnz;
  if (n_distinct) *n_distinct = m->n_distinct;
  if (device_bytes) *device_bytes = m->bytes;
  return MSM_AMD_OK;
}

int msm_amd_fr_matrix_free(msm_amd_ctx* ctx, msm_amd_fr_matrix* matrix) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return handle_free(ctx, ctx->live_fr_mat, matrix, "msm_amd_fr_matrix_free: not a matrix handle of this ctx");
}

int msm_amd_fr_matvec(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, int scalar_layout, const void* x, void* y) {
  return fr_matvec_call(ctx, matrix, true, scalar_layout, x, y, nullptr);
}

int msm_amd_fr_matvec_device(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, int scalar_layout, const void* d_x, void* d_y,
                             float* kernel_ms) {
  return fr_matvec_call(ctx, matrix, false, scalar_layout, d_x, d_y, kernel_ms);
}

}  // extern "C"

// ---- multilinear tables over Fr and sumcheck rounds (msm_amd_fr_mle_bind*, msm_amd_fr_mle_eval*, msm_amd_fr_eq_table*,
// msm_amd_fr_sumcheck_round*, _round_terms*, _step_terms*) ------------------------------------------------------------------------------------------------
// Through device_call.  Challenges and points are read once on the host and reach the kernels by value.  The values of an
// evaluation or a round come back through CallState::h_values.  The host form of a bind copies back the records the call
// defines and no byte between the tables: one strided copy behind the kernels.
namespace {

int fr_mle_bind_call(msm_amd_ctx* ctx, bool host, int scalar_layout, int order, const void* r32, size_t n_bind, const void* in,
                     size_t n, size_t n_vec, size_t stride, void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_mle_bind" : "msm_amd_fr_mle_bind_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_mle_bind_check(scalar_layout, order, r32, n_bind, in, n, n_vec, stride, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrMleBindLaunch c{};
  c.n = n, c.n_vec = n_vec, c.stride = stride, c.n_bind = (uint32_t)n_bind, c.layout = scalar_layout, c.order = order;
  for (size_t k = 0; k < n_bind; ++k) c.r[k] = fr_read_record(scalar_layout, (const uint8_t*)r32 + k * 32);
  const FrMleBindPlan plan = fr_mle_bind_plan(order, n, n_vec, c.n_bind);
  const size_t span = ((n_vec - 1) * stride + n) * 32, left = (n >> n_bind) * 32;
  // the host form works from the staged input into the staged output; the strided copy below brings the result back
  d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = span;
  d.out = out;
  d.work[0] = {&s.work, std::max<size_t>(32, plan.work_records * 32)};
  if (host) d.work[1] = {&s.out, span};
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) -> int {
    c.in = io.in[0], c.out = host ? s.out.p : io.out, c.work = s.work.p;
    launch_fr_mle_bind(st, c);
    if (host)
      HIP_TRY(ctx, hipMemcpy2DAsync(out, stride * 32, s.out.p, stride * 32, left, n_vec, hipMemcpyDeviceToHost, st));
    return MSM_AMD_OK;
  });
}

int fr_mle_eval_call(msm_amd_ctx* ctx, bool host, int scalar_layout, int order, const void* point32, const void* in, size_t n,
                     size_t n_vec, size_t stride, void* y_out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_mle_eval" : "msm_amd_fr_mle_eval_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_mle_eval_check(scalar_layout, order, point32, in, n, n_vec, stride, y_out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrMleEvalLaunch c{};
  c.n = n, c.n_vec = n_vec, c.stride = stride, c.tile_log = ctx->fr_tile_log, c.layout = scalar_layout;
  const uint32_t m = fr_mle_log2(n);
  // the kernels fold x_j at r[j]: HIGH binds x_(m-1-s) at point[s]
  for (uint32_t k = 0; k < m; ++k)
    c.r[order == kFrMleHigh ? m - 1 - k : k] = fr_read_record(scalar_layout, (const uint8_t*)point32 + (size_t)k * 32);
  const FrScanPlan plan = fr_scan_plan(n, n_vec, c.tile_log);
  d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = ((n_vec - 1) * stride + n) * 32;
  d.work[0] = {&s.work, fr_poly_values(plan) + n_vec * 32};
  d.values_bytes = n_vec * 32;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
    c.in = io.in[0], c.work = s.work.p;
    launch_fr_mle_eval(st, c);
    io.values = (const uint8_t*)s.work.p + fr_poly_values(plan);
    return MSM_AMD_OK;
  });
  if (rc == MSM_AMD_OK) fr_values_out(s, scalar_layout, n_vec, y_out);
  return rc;
}

int fr_eq_table_call(msm_amd_ctx* ctx, bool host, int scalar_layout, int order, const void* point32, size_t m, void* out,
                     float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_eq_table" : "msm_amd_fr_eq_table_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_eq_table_check(scalar_layout, order, point32, m, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  std::lock_guard<std::mutex> lk(ctx->mu);
  u256 by_bit[kFrMleMaxVars];
  for (size_t k = 0; k < m; ++k)
    by_bit[order == kFrMleHigh ? m - 1 - k : k] = fr_read_record(scalar_layout, (const uint8_t*)point32 + k * 32);
  d.host = host, d.kernel_ms = kernel_ms;
  d.out = out, d.out_bytes = ((size_t)1 << m) * 32;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_fr_eq_table(st, scalar_layout, by_bit, (uint32_t)m, io.out);
    return MSM_AMD_OK;
  });
}

int fr_sumcheck_round_call(msm_amd_ctx* ctx, bool host, int scalar_layout, int order, int form, const void* in, size_t n,
                           size_t n_vec, size_t stride, void* g_out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_sumcheck_round" : "msm_amd_fr_sumcheck_round_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (const char* why = fr_sumcheck_check(scalar_layout, order, form, in, n, n_vec, stride, g_out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrMleRoundLaunch c{};
  c.n = n, c.n_vec = n_vec, c.stride = stride, c.chunk_log = ctx->fr_mle_chunk_log;
  c.layout = scalar_layout, c.order = order, c.form = form;
  const uint32_t values = fr_mle_degree(form, n_vec) + 1;
  const FrMleRoundPlan plan = fr_mle_round_plan(n, values, c.chunk_log);
  d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = ((n_vec - 1) * stride + n) * 32;
  d.work[0] = {&s.work, plan.records * 32};
  d.values_bytes = values * 32;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
    c.in = io.in[0], c.work = s.work.p;
    launch_fr_sumcheck_round(st, c);
    io.values = (const uint8_t*)s.work.p + plan.values_off * 32;
    return MSM_AMD_OK;
  });
  if (rc == MSM_AMD_OK) fr_values_out(s, scalar_layout, values, g_out);
  return rc;
}

// A round over a term list, and the step: the bind launch of every table at r and the round launch over what it wrote, on
// the stream under the call's one wait (a kernel that folds and sums in one pass was measured and is slower than the two
// launches at every size: DESIGN.md section 8.17).  The host
// form of the step works from the staged input into the staged output and brings back the n / 2 records of every table the
// call defines, as the host form of a bind does.
int fr_sumcheck_terms_call(msm_amd_ctx* ctx, int mem, bool step, int scalar_layout, int order,
                           const msm_amd_fr_sumcheck_terms* terms, const void* r32, const void* in, size_t n, size_t n_vec,
                           size_t stride, void* out, void* g_out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = step ? "msm_amd_fr_sumcheck_step_terms" : "msm_amd_fr_sumcheck_round_terms";
  if (kernel_ms) *kernel_ms = 0.f;
  if (mem != MSM_AMD_MEM_HOST && mem != MSM_AMD_MEM_DEVICE)
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": mem must be MSM_AMD_MEM_HOST or MSM_AMD_MEM_DEVICE");
  const bool host = mem == MSM_AMD_MEM_HOST;
  FrTermRoundLaunch c{};
  if (const char* why = step ? fr_sumcheck_step_check(scalar_layout, order, terms, r32, in, n, n_vec, stride, out, g_out, !host, &c.terms)
                             : fr_sumcheck_terms_round_check(scalar_layout, order, terms, in, n, n_vec, stride, g_out, !host, &c.terms))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  c.n = n, c.n_vec = n_vec, c.stride = stride, c.chunk_log = ctx->fr_mle_chunk_log;
  c.layout = scalar_layout, c.order = order, c.step = step;
  if (step) c.r = fr_read_record(scalar_layout, r32);
  const uint32_t values = fr_sum_degree(c.terms) + 1;
  const FrMleRoundPlan plan = fr_mle_round_plan(step ? n / 2 : n, values, c.chunk_log);
  const size_t span = ((n_vec - 1) * stride + n) * 32;
  d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = span;
  d.out = out;
  d.work[0] = {&s.work, plan.records * 32};
  if (host && step) d.work[1] = {&s.out, span};
  d.values_bytes = values * 32;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) -> int {
    c.in = io.in[0], c.out = !step ? nullptr : host ? s.out.p : io.out, c.work = s.work.p;
    launch_fr_sumcheck_terms(st, c);
    if (host && step)
      HIP_TRY(ctx, hipMemcpy2DAsync(out, stride * 32, s.out.p, stride * 32, n / 2 * 32, n_vec, hipMemcpyDeviceToHost, st));
    io.values = (const uint8_t*)s.work.p + plan.values_off * 32;
    return MSM_AMD_OK;
  });
  if (rc == MSM_AMD_OK) fr_values_out(s, scalar_layout, values, g_out);
  return rc;
}

// A gate polynomial over rotated columns: one launch.  The host form stages the columns, and with ACCUMULATE the old
// records of out as the second input; the result leaves through the staged output.  The scale table is host memory in
// either form: it is reduced here and goes up as the third input into ctx-owned memory.
int fr_gate_call(msm_amd_ctx* ctx, int mem, int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms, const void* in,
                 size_t n, size_t n_vec, size_t stride, uint64_t rot_step, const void* k_acc32, const void* scale, size_t period,
                 void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = "msm_amd_fr_gate_eval";
  if (kernel_ms) *kernel_ms = 0.f;
  FrGateLaunch c{};
  if (const char* why = fr_gate_eval_check(mem, scalar_layout, flags, terms, in, n, n_vec, stride, rot_step, k_acc32, scale, period,
                                           out, &c.terms))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  const bool host = mem == MSM_AMD_MEM_HOST;
  std::lock_guard<std::mutex> lk(ctx->mu);
  c.n = n, c.stride = stride, c.layout = scalar_layout, c.accumulate = flags & kFrGateAccumulate;
  if (c.accumulate) c.k_acc = fr_read_record(scalar_layout, k_acc32);
  std::vector<u256> table(scale ? period : 0);
  for (size_t j = 0; j < table.size(); ++j) table[j] = fr_read_record(scalar_layout, (const uint8_t*)scale + j * 32);
  c.period = scale ? (uint32_t)period : 1;
  d.host = host, d.host_in = (host ? 1u | (c.accumulate ? 2u : 0u) : 0u) | (scale ? 4u : 0u), d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = ((n_vec - 1) * stride + n) * 32;
  if (c.accumulate) d.in[1] = out, d.in_bytes[1] = n * 32;
  if (scale) d.in[2] = table.data(), d.in_bytes[2] = period * 32;
  d.out = out, d.out_bytes = n * 32;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    c.in = io.in[0], c.acc = c.accumulate ? io.in[1] : nullptr, c.scale = scale ? io.in[2] : nullptr, c.out = io.out;
    launch_fr_gate(st, c);
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_fr_gate_eval(msm_amd_ctx* ctx, int mem, int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms,
                         const void* in, size_t n, size_t n_vec, size_t stride, uint64_t rot_step, const void* k_acc32,
                         const void* scale, size_t period, void* out, float* kernel_ms) {
  return fr_gate_call(ctx, mem, scalar_layout, flags, terms, in, n, n_vec, stride, rot_step, k_acc32, scale, period, out,
                      kernel_ms);
}

int msm_amd_fr_mle_bind(msm_amd_ctx* ctx, int scalar_layout, int order, const void* r, size_t n_bind, const void* in, size_t n,
                        size_t n_vec, size_t stride, void* out) {
  return fr_mle_bind_call(ctx, true, scalar_layout, order, r, n_bind, in, n, n_vec, stride, out, nullptr);
}

int msm_amd_fr_mle_bind_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* r, size_t n_bind, const void* d_in,
                               size_t n, size_t n_vec, size_t stride, void* d_out, float* kernel_ms) {
  return fr_mle_bind_call(ctx, false, scalar_layout, order, r, n_bind, d_in, n, n_vec, stride, d_out, kernel_ms);
}

int msm_amd_fr_mle_eval(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point, const void* in, size_t n,
                        size_t n_vec, size_t stride, void* y_out) {
  return fr_mle_eval_call(ctx, true, scalar_layout, order, point, in, n, n_vec, stride, y_out, nullptr);
}

int msm_amd_fr_mle_eval_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point, const void* d_in, size_t n,
                               size_t n_vec, size_t stride, void* y_out, float* kernel_ms) {
  return fr_mle_eval_call(ctx, false, scalar_layout, order, point, d_in, n, n_vec, stride, y_out, kernel_ms);
}

int msm_amd_fr_eq_table(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point, size_t m, void* out) {
  return fr_eq_table_call(ctx, true, scalar_layout, order, point, m, out, nullptr);
}

int msm_amd_fr_eq_table_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point, size_t m, void* d_out,
                               float* kernel_ms) {
  return fr_eq_table_call(ctx, false, scalar_layout, order, point, m, d_out, kernel_ms);
}

int msm_amd_fr_sumcheck_round(msm_amd_ctx* ctx, int scalar_layout, int order, int form, const void* in, size_t n, size_t n_vec,
                              size_t stride, void* g_out) {
  return fr_sumcheck_round_call(ctx, true, scalar_layout, order, form, in, n, n_vec, stride, g_out, nullptr);
}

int msm_amd_fr_sumcheck_round_device(msm_amd_ctx* ctx, int scalar_layout, int order, int form, const void* d_in, size_t n,
                                     size_t n_vec, size_t stride, void* g_out, float* kernel_ms) {
  return fr_sumcheck_round_call(ctx, false, scalar_layout, order, form, d_in, n, n_vec, stride, g_out, kernel_ms);
}

int msm_amd_fr_sumcheck_round_terms(msm_amd_ctx* ctx, int mem, int scalar_layout, int order,
                                    const msm_amd_fr_sumcheck_terms* terms, const void* in, size_t n, size_t n_vec,
                                    size_t stride, void* g_out, float* kernel_ms) {
  return fr_sumcheck_terms_call(ctx, mem, false, scalar_layout, order, terms, nullptr, in, n, n_vec, stride, nullptr, g_out, kernel_ms);
}

int msm_amd_fr_sumcheck_step_terms(msm_amd_ctx* ctx, int mem, int scalar_layout, int order,
                                   const msm_amd_fr_sumcheck_terms* terms, const void* r, const void* in, size_t n, size_t n_vec,
                                   size_t stride, void* out, void* g_out, float* kernel_ms) {
  return fr_sumcheck_terms_call(ctx, mem, true, scalar_layout, order, terms, r, in, n, n_vec, stride, out, g_out, kernel_ms);
}

}  // extern "C"

// ---- width scan (msm_amd_scalar_width*): through device_call; the 32-byte result comes back as the call's values ----------
namespace {

int scalar_width_call(msm_amd_ctx* ctx, bool host, int scalar_layout, const void* scalars, size_t n, int sign, uint32_t* bits,
                      uint64_t* stats) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_scalar_width" : "msm_amd_scalar_width_device";
  if (const char* why = scalar_width_check(scalar_layout, scalars, n, sign, bits))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  WidthStats r;
  if (n != 0) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    CallState& s = ctx->calls;
    d.host_in = host ? 1u : 0u;
    d.in[0] = scalars, d.in_bytes[0] = n * 32;
    d.work[0] = {&s.work, scalar_width_work_bytes(n)};
    d.values_bytes = 32;
    const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
      launch_scalar_width(st, (const u256*)io.in[0], (uint32_t)n, scalar_layout == MSM_AMD_SCALAR_MONT_LE, (uint32_t)sign,
                          s.work.p);
      io.values = s.work.p;
      return MSM_AMD_OK;
    });
    if (rc) return rc;
    uint64_t v[4];
    std::memcpy(v, s.h_values, 32);
    r.bits = (uint32_t)(v[0] >> 32), r.widest = (uint32_t)~(uint32_t)v[0], r.zeros = v[1], r.negatives = v[2];
  }
  scalar_width_out(r, bits, stats);
  return MSM_AMD_OK;
}

}  // namespace

extern "C" {

int msm_amd_scalar_width(msm_amd_ctx* ctx, int scalar_layout, const void* scalars, size_t n, int sign, uint32_t* bits,
                         uint64_t* stats) {
  return scalar_width_call(ctx, true, scalar_layout, scalars, n, sign, bits, stats);
}
int msm_amd_scalar_width_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_scalars, size_t n, int sign, uint32_t* bits,
                                uint64_t* stats) {
  return scalar_width_call(ctx, false, scalar_layout, d_scalars, n, sign, bits, stats);
}

}  // extern "C"

// ---- Poseidon over Fr (msm_amd_poseidon_params_*, msm_amd_poseidon_permute*, _hash*, _merkle_build*, _merkle_paths*) ---------
// Through device_call.  A parameter handle is validated by membership in ctx->live_poseidon, under the lock and before
// anything is sized by it; the tag is read once on the host and reaches the kernels by value; the root of a tree comes back
// through CallState::h_values in the call's one bounded wait; the leaf indices of a paths call are checked on the host and
// go through the staging in both forms.
namespace {

const char* const kNotPoseidon = ": not a Poseidon parameter handle of this ctx";

PoseidonLaunch poseidon_launch(const msm_amd_poseidon_params* p, int scalar_layout, const void* tag32) {
  PoseidonLaunch c{};
  c.image = p->d_mem, c.t = p->t, c.r_f = p->r_f, c.r_p = p->r_p, c.layout = scalar_layout;
  c.tag = tag32 ? fr_read_record(scalar_layout, tag32) : u256_zero();
  return c;
}

// device memory a call writes must not be the constants
bool poseidon_clear_of(const msm_amd_poseidon_params* p, const void* out, size_t bytes) {
  const uintptr_t lo = (uintptr_t)p->d_mem, hi = lo + p->bytes, a = (uintptr_t)out;
  return !(a < hi && lo < a + bytes);
}

int poseidon_call(msm_amd_ctx* ctx, const msm_amd_poseidon_params* handle, int kind, bool host, int scalar_layout,
                  const void* tag32, const void* in, size_t n, void* out, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = std::string(kind == kPoseidonHash ? "msm_amd_poseidon_hash" : "msm_amd_poseidon_permute") + (host ? "" : "_device");
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_poseidon_params* p = find_handle(ctx->live_poseidon, handle);
  if (!p) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + kNotPoseidon);
  if (const char* why = poseidon_call_check(kind, p->t, scalar_layout, in, n, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0) return MSM_AMD_OK;
  const size_t in_bytes = n * (kind == kPoseidonHash ? p->t - 1 : p->t) * 32, out_bytes = n * (kind == kPoseidonHash ? 1 : p->t) * 32;
  if (!host && !poseidon_clear_of(p, out, out_bytes))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": the output must not overlap the parameters");
  const PoseidonLaunch c = poseidon_launch(p, scalar_layout, tag32);
  // the host form of a permutation works in place on the staged copy of its input
  d.host = host, d.host_in = host, d.in_place = host && kind == kPoseidonPermute, d.kernel_ms = kernel_ms;
  d.in[0] = in, d.in_bytes[0] = in_bytes;
  d.out = out, d.out_bytes = out_bytes;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_poseidon(st, c, kind, io.in[0], n, io.out);
    return MSM_AMD_OK;
  });
}

int poseidon_merkle_build_call(msm_amd_ctx* ctx, const msm_amd_poseidon_params* handle, bool host, int scalar_layout,
                               const void* tag32, const void* leaves, size_t n_leaves, void* tree, void* root32, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_poseidon_merkle_build" : "msm_amd_poseidon_merkle_build_device";
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_poseidon_params* p = find_handle(ctx->live_poseidon, handle);
  if (!p) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + kNotPoseidon);
  if (const char* why = poseidon_merkle_check(p->t, scalar_layout, leaves, n_leaves, tree, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  const PoseidonTreePlan plan = poseidon_tree_plan(n_leaves, p->t - 1, ctx->poseidon_top_log);
  if (!host && !poseidon_clear_of(p, tree, plan.nodes * 32))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": the tree must not overlap the parameters");
  const PoseidonLaunch c = poseidon_launch(p, scalar_layout, tag32);
  CallState& s = ctx->calls;
  d.host = host, d.host_in = host, d.kernel_ms = kernel_ms;
  d.in[0] = leaves, d.in_bytes[0] = n_leaves * 32;
  d.out = tree, d.out_bytes = plan.nodes * 32;
  d.values_bytes = root32 ? 32 : 0;
  const int rc = device_call(ctx, d, [&](hipStream_t st, CallIo& io) {
    launch_poseidon_tree(st, c, io.in[0], n_leaves, ctx->poseidon_top_log, io.out);
    io.values = (const uint8_t*)io.out + (plan.nodes - 1) * 32;
    return MSM_AMD_OK;
  });
  if (rc == MSM_AMD_OK && root32) std::memcpy(root32, s.h_values, 32);   // a node: already in the call's layout
  return rc;
}

int poseidon_merkle_paths_call(msm_amd_ctx* ctx, const msm_amd_poseidon_params* handle, bool host, int scalar_layout,
                               const void* leaves, size_t n_leaves, const void* tree, const uint64_t* idx, size_t n_idx, void* out,
                               float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_poseidon_merkle_paths" : "msm_amd_poseidon_merkle_paths_device";
  if (kernel_ms) *kernel_ms = 0.f;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_poseidon_params* p = find_handle(ctx->live_poseidon, handle);
  if (!p) return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + kNotPoseidon);
  if (const char* why = poseidon_paths_check(p->t, scalar_layout, leaves, n_leaves, tree, idx, n_idx, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n_idx == 0) return MSM_AMD_OK;
  const uint32_t arity = p->t - 1, depth = poseidon_tree_depth(n_leaves, arity);
  const size_t nodes = (n_leaves - 1) / (arity - 1), out_bytes = n_idx * depth * (arity - 1) * 32;
  if (!host && !poseidon_clear_of(p, out, out_bytes))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": the paths must not overlap the parameters");
  d.host = host, d.host_in = host ? 7u : 4u, d.kernel_ms = kernel_ms;
  d.in[0] = leaves, d.in_bytes[0] = n_leaves * 32;
  d.in[1] = tree, d.in_bytes[1] = nodes * 32;
  d.in[2] = idx, d.in_bytes[2] = n_idx * sizeof(uint64_t);
  d.out = out, d.out_bytes = out_bytes;
  return device_call(ctx, d, [&](hipStream_t st, const CallIo& io) {
    launch_merkle_paths(st, scalar_layout, arity, depth, io.in[0], n_leaves, io.in[1], io.in[2], n_idx, io.out);
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_poseidon_params_build(msm_amd_ctx* ctx, uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark,
                                  const void* mds, msm_amd_poseidon_params** out) {
  if (!ctx || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_poseidon_params_build: null pointer");
  *out = nullptr;
  if (const char* why = poseidon_constants_check(t, r_f, r_p, scalar_layout, ark, mds))
    return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_poseidon_params_build: ") + why);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  std::vector<u256> image;
  poseidon_build_image(t, r_f, r_p, scalar_layout, ark, mds, &image);
  int up = MSM_AMD_OK;
  if (int rc = handle_build_tail(ctx, ctx->live_poseidon, image.size() * 32, "the constants of a Poseidon instance",
                                 "Poseidon parameter build",
                                 [&](void* d_mem) { up = staged_upload(ctx, d_mem, image.data(), image.size() * 32, ctx->stream); },
                                 out))
    return rc;
  if (up) {   // the upload did not go through: nothing may read the allocation
    msm_amd_poseidon_params* h = *out;
    *out = nullptr;
    const std::string why = ctx->last_error;
    handle_free(ctx, ctx->live_poseidon, h, "");
    return fail(ctx, up, "msm_amd_poseidon_params_build: " + why);
  }
  (*out)->t = t, (*out)->r_f = r_f, (*out)->r_p = r_p;
  return MSM_AMD_OK;
}

int msm_amd_poseidon_params_info(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, uint32_t* t, uint32_t* r_f,
                                 uint32_t* r_p, size_t* device_bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_poseidon_params* p = find_handle(ctx->live_poseidon, params);
  if (!p) return fail(ctx, MSM_AMD_INPUT_ERROR, std::string("msm_amd_poseidon_params_info") + kNotPoseidon);
  if (t) *t = p->t;
  if (r_f) *r_f = p->r_f;
  if (r_p) *r_p = p->r_p;
  if (device_bytes) *device_bytes = p->bytes;
  return MSM_AMD_OK;
}

int msm_amd_poseidon_params_free(msm_amd_ctx* ctx, msm_amd_poseidon_params* params) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return handle_free(ctx, ctx->live_poseidon, params, "msm_amd_poseidon_params_free: not a Poseidon parameter handle of this ctx");
}

int msm_amd_poseidon_permute(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* in, size_t n,
                             void* out) {
  return poseidon_call(ctx, params, kPoseidonPermute, true, scalar_layout, nullptr, in, n, out, nullptr);
}

int msm_amd_poseidon_permute_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* d_in,
                                    size_t n, void* d_out, float* kernel_ms) {
  return poseidon_call(ctx, params, kPoseidonPermute, false, scalar_layout, nullptr, d_in, n, d_out, kernel_ms);
}

int msm_amd_poseidon_hash(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* tag32,
                          const void* in, size_t n, void* out) {
  return poseidon_call(ctx, params, kPoseidonHash, true, scalar_layout, tag32, in, n, out, nullptr);
}

int msm_amd_poseidon_hash_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* tag32,
                                 const void* d_in, size_t n, void* d_out, float* kernel_ms) {
  return poseidon_call(ctx, params, kPoseidonHash, false, scalar_layout, tag32, d_in, n, d_out, kernel_ms);
}

int msm_amd_poseidon_merkle_build(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* tag32,
                                  const void* leaves, size_t n_leaves, void* tree, void* root32) {
  return poseidon_merkle_build_call(ctx, params, true, scalar_layout, tag32, leaves, n_leaves, tree, root32, nullptr);
}

int msm_amd_poseidon_merkle_build_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout,
                                         const void* tag32, const void* d_leaves, size_t n_leaves, void* d_tree, void* root32,
                                         float* kernel_ms) {
  return poseidon_merkle_build_call(ctx, params, false, scalar_layout, tag32, d_leaves, n_leaves, d_tree, root32, kernel_ms);
}

int msm_amd_poseidon_merkle_paths(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* leaves,
                                  size_t n_leaves, const void* tree, const uint64_t* idx, size_t n_idx, void* out) {
  return poseidon_merkle_paths_call(ctx, params, true, scalar_layout, leaves, n_leaves, tree, idx, n_idx, out, nullptr);
}

int msm_amd_poseidon_merkle_paths_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout,
                                         const void* d_leaves, size_t n_leaves, const void* d_tree, const uint64_t* idx,
                                         size_t n_idx, void* d_out, float* kernel_ms) {
  return poseidon_merkle_paths_call(ctx, params, false, scalar_layout, d_leaves, n_leaves, d_tree, idx, n_idx, d_out, kernel_ms);
}

}  // extern "C"
