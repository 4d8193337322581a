// The blocking point calls of both groups (device_call.h): validation, compressed points, batch scalar multiplication
// with its stage entries, the transform over G1 points with its levels tap, and the pairing calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "device_call.h"
#include "launch_compress.h"
#include "launch_mul.h"
#include "launch_nttp.h"
#include "host_pairing.h"
#include "launch_pairing.h"

namespace {

// ---- point validation (msm_amd_check_points*, msm_amd_g2_check_points*) ---------------------------------------------
int check_call(msm_amd_ctx* ctx, bool g2, bool host, int layout, const void* points, size_t n, uint32_t checks,
               uint8_t* reasons, msm_amd_check_report* report) {
  if (!ctx || !report) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = g2 ? "msm_amd_g2_check_points" : "msm_amd_check_points";   // the _device calls go by the same name
  const uint32_t stride = point_record_bytes(g2, layout, kKindHost);
  if (stride == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": takes the host point layouts only (not *_PREPARED / *_TABLES)");
  if (checks == 0 || (checks & ~(uint32_t)(MSM_AMD_CHECK_CURVE | MSM_AMD_CHECK_SUBGROUP)))
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": checks must be MSM_AMD_CHECK_CURVE and / or MSM_AMD_CHECK_SUBGROUP");
  c.g2 = g2, c.counters = true, c.n = n;
  c.all_host(host);
  c.in[0] = points, c.in_bytes[0] = n * stride;
  c.reasons = reasons;
  if (g2) c.stage[0] = &ctx->g2.in_points;
  return point_call(
      ctx, c, !points,
      [&](hipStream_t st, const CallIo& io) {
        if (g2)
          launch_check_g2(st, io.in[0], layout == MSM_AMD_G2_POINT_ARK_AFFINE, (uint32_t)n, checks, io.reasons, io.counters);
        else
          launch_check_g1(st, io.in[0], layout, stride, (uint32_t)n, io.reasons, io.counters);
        return MSM_AMD_OK;
      },
      [&](const PointCounters& pc, float ms) { point_report_decode(pc, n, ms, report); });
}

// ---- compressed points (msm_amd_decompress_points*, msm_amd_compress_points* and their G2 forms) ----------------------
// layout: the output layout of a decompression, the input layout of a compression
int compress_call(msm_amd_ctx* ctx, bool g2, bool host, bool decompress, int format, int layout, const void* in, size_t n,
                  void* out, uint8_t* reasons, msm_amd_decompress_report* report, uint64_t* n_bad) {
  if (!ctx || (decompress && !report)) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = std::string(g2 ? "msm_amd_g2_" : "msm_amd_") + (decompress ? "decompress_points" : "compress_points") +
          (host ? "" : "_device");
  const bool prepared_ok = decompress && !host;
  const uint32_t stride = point_record_bytes(g2, layout, prepared_ok ? kKindAffine | kKindPrepared : kKindAffine);
  if (!compress_format_known(format))
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": unknown format (MSM_AMD_COMPRESSED_ARK / _PARITY)");
  if (stride == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + (prepared_ok ? ": takes the two affine layouts and *_PREPARED (not *_TABLES)"
                                                               : ": takes the two affine host layouts only"));
  const size_t wire = g2 ? 64 : 32;
  c.g2 = g2, c.counters = true, c.n = n;
  c.all_host(host);
  c.in[0] = in, c.in_bytes[0] = n * (decompress ? wire : stride);
  c.out = out, c.out_bytes = n * (decompress ? stride : wire);
  c.reasons = reasons;
  return point_call(
      ctx, c, !in || !out,
      [&](hipStream_t st, const CallIo& io) {
        if (decompress)
          launch_decompress(st, g2, format, io.in[0], (uint32_t)n, layout, stride, io.out, io.reasons, io.counters);
        else
          launch_compress(st, g2, layout, stride, io.in[0], (uint32_t)n, format, io.out, io.counters);
        return MSM_AMD_OK;
      },
      [&](const PointCounters& pc, float ms) {
        if (decompress) point_report_decode(pc, n, ms, report);
        else if (n_bad) *n_bad = pc.by_reason[kPointNotReduced];
      });
}

// ---- batch scalar multiplication (msm_amd_mul_points*, msm_amd_g2_mul_points*) ------------------------------------------
// The outputs run in chunks of ctx->mul_chunk records (a multiple of the normalisation group, so the groups of a
// chunked call are those of an unchunked one), all enqueued on the main stream: stream order hands the XYZZ buffer from
// one chunk to the next.  No counters and no event: the bounded stream wait at the end of device_call is the call's.
int mul_call(msm_amd_ctx* ctx, bool g2, bool host, int scalar_layout, int layout_in, int base_mode, const void* scalars,
             const void* points, size_t n, int layout_out, void* out) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = std::string(g2 ? "msm_amd_g2_mul_points" : "msm_amd_mul_points") + (host ? "" : "_device");
  const uint32_t prepared = host ? 0u : (uint32_t)kKindPrepared;
  const size_t in_stride = point_record_bytes(g2, layout_in, kKindHost | prepared),
               out_stride = point_record_bytes(g2, layout_out, kKindAffine | prepared);
  if (!mul_scalar_layout_known(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": unknown scalar layout");
  if (in_stride == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + (host ? ": points in a host layout only (not *_PREPARED / *_TABLES)"
                                                        : ": points in a host layout or *_PREPARED (not *_TABLES)"));
  if (out_stride == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + (host ? ": output in one of the two affine host layouts only"
                                                        : ": output in one of the two affine layouts or *_PREPARED"));
  if (base_mode != MSM_AMD_MUL_BASE_EACH && base_mode != MSM_AMD_MUL_BASE_ONE)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": base_mode must be MSM_AMD_MUL_BASE_EACH or MSM_AMD_MUL_BASE_ONE");
  const bool one = base_mode == MSM_AMD_MUL_BASE_ONE;
  const size_t chunk = std::min(n, ctx->mul_chunk);
  CallState& s = g2 ? ctx->g2.calls : ctx->calls;
  c.g2 = g2, c.n = n;
  c.all_host(host);
  c.in[0] = scalars, c.in_bytes[0] = n * 32;
  c.in[1] = points, c.in_bytes[1] = (one ? 1 : n) * in_stride;
  c.out = out, c.out_bytes = n * out_stride;
  c.work[0] = {&s.table, one ? mul_table_bytes(g2) : 0}, c.work[1] = {&s.xyzz, chunk * mul_xyzz_bytes(g2)};
  return point_call(
      ctx, c, !scalars || !points || !out,
      [&](hipStream_t st, const CallIo& io) {
        void *table = s.table.p, *xyzz = s.xyzz.p;
        if (one) launch_mul_table(st, g2, layout_in, io.in[1], table);
        for (size_t first = 0; first < n; first += chunk) {
          const uint32_t m = (uint32_t)std::min(chunk, n - first);
          const uint8_t* sc = (const uint8_t*)io.in[0] + first * 32;
          if (one)
            launch_mul_fixed(st, g2, scalar_layout, sc, m, table, xyzz);
          else
            launch_mul_each(st, g2, scalar_layout, sc, layout_in, (const uint8_t*)io.in[1] + first * in_stride, m, xyzz);
          launch_mul_normalise(st, g2, xyzz, m, layout_out, (uint8_t*)io.out + first * out_stride);
        }
        return MSM_AMD_OK;
      },
      [](const PointCounters&, float) {});
}

}  // namespace

extern "C" {

int msm_amd_check_points(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, uint32_t checks,
                         uint8_t* reasons, msm_amd_check_report* report) {
  return check_call(ctx, false, true, point_layout, points, n, checks, reasons, report);
}

int msm_amd_check_points_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, uint32_t checks,
                                uint8_t* d_reasons, msm_amd_check_report* report) {
  return check_call(ctx, false, false, point_layout, d_points, n, checks, d_reasons, report);
}

int msm_amd_g2_check_points(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, uint32_t checks,
                            uint8_t* reasons, msm_amd_check_report* report) {
  return check_call(ctx, true, true, g2_point_layout, points, n, checks, reasons, report);
}

int msm_amd_g2_check_points_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                   uint32_t checks, uint8_t* d_reasons, msm_amd_check_report* report) {
  return check_call(ctx, true, false, g2_point_layout, d_points, n, checks, d_reasons, report);
}

int msm_amd_decompress_points(msm_amd_ctx* ctx, int format, const void* in, size_t n, int point_layout_out, void* out,
                              uint8_t* reasons, msm_amd_decompress_report* report) {
  return compress_call(ctx, false, true, true, format, point_layout_out, in, n, out, reasons, report, nullptr);
}

int msm_amd_decompress_points_device(msm_amd_ctx* ctx, int format, const void* d_in, size_t n, int point_layout_out,
                                     void* d_out, uint8_t* d_reasons, msm_amd_decompress_report* report) {
  return compress_call(ctx, false, false, true, format, point_layout_out, d_in, n, d_out, d_reasons, report, nullptr);
}

int msm_amd_g2_decompress_points(msm_amd_ctx* ctx, int format, const void* in, size_t n, int g2_point_layout_out,
                                 void* out, uint8_t* reasons, msm_amd_decompress_report* report) {
  return compress_call(ctx, true, true, true, format, g2_point_layout_out, in, n, out, reasons, report, nullptr);
}

int msm_amd_g2_decompress_points_device(msm_amd_ctx* ctx, int format, const void* d_in, size_t n,
                                        int g2_point_layout_out, void* d_out, uint8_t* d_reasons,
                                        msm_amd_decompress_report* report) {
  return compress_call(ctx, true, false, true, format, g2_point_layout_out, d_in, n, d_out, d_reasons, report, nullptr);
}

int msm_amd_compress_points(msm_amd_ctx* ctx, int point_layout_in, const void* in, size_t n, int format, void* out,
                            uint64_t* n_bad) {
  return compress_call(ctx, false, true, false, format, point_layout_in, in, n, out, nullptr, nullptr, n_bad);
}

int msm_amd_compress_points_device(msm_amd_ctx* ctx, int point_layout_in, const void* d_in, size_t n, int format,
                                   void* d_out, uint64_t* n_bad) {
  return compress_call(ctx, false, false, false, format, point_layout_in, d_in, n, d_out, nullptr, nullptr, n_bad);
}

int msm_amd_g2_compress_points(msm_amd_ctx* ctx, int g2_point_layout_in, const void* in, size_t n, int format, void* out,
                               uint64_t* n_bad) {
  return compress_call(ctx, true, true, false, format, g2_point_layout_in, in, n, out, nullptr, nullptr, n_bad);
}

int msm_amd_g2_compress_points_device(msm_amd_ctx* ctx, int g2_point_layout_in, const void* d_in, size_t n, int format,
                                      void* d_out, uint64_t* n_bad) {
  return compress_call(ctx, true, false, false, format, g2_point_layout_in, d_in, n, d_out, nullptr, nullptr, n_bad);
}

int msm_amd_mul_points(msm_amd_ctx* ctx, int scalar_layout, int point_layout_in, int base_mode, const void* scalars,
                       const void* points, size_t n, int point_layout_out, void* out) {
  return mul_call(ctx, false, true, scalar_layout, point_layout_in, base_mode, scalars, points, n, point_layout_out, out);
}

int msm_amd_mul_points_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout_in, int base_mode,
                              const void* d_scalars, const void* d_points, size_t n, int point_layout_out, void* d_out) {
  return mul_call(ctx, false, false, scalar_layout, point_layout_in, base_mode, d_scalars, d_points, n, point_layout_out,
                  d_out);
}

int msm_amd_g2_mul_points(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout_in, int base_mode, const void* scalars,
                          const void* points, size_t n, int g2_point_layout_out, void* out) {
  return mul_call(ctx, true, true, scalar_layout, g2_point_layout_in, base_mode, scalars, points, n, g2_point_layout_out,
                  out);
}

int msm_amd_g2_mul_points_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout_in, int base_mode,
                                 const void* d_scalars, const void* d_points, size_t n, int g2_point_layout_out,
                                 void* d_out) {
  return mul_call(ctx, true, false, scalar_layout, g2_point_layout_in, base_mode, d_scalars, d_points, n,
                  g2_point_layout_out, d_out);
}

}  // extern "C"

// ---- stage entries of the batch scalar multiplication (test aid: msm_amd_test_mul_stage, msm_amd_test_mul_stage_host) ----
// The digit walk and the shared normalisation of mul_points.hip.h on inputs the public calls never produce: a table the
// caller wrote (identity entries, an entry equal to a partial sum or to its negative) and XYZZ records at the edge of
// the point invariant.  The device form goes through point_call (device_call) and the launch wrappers of launch_mul.h like
// msm_amd_mul_points; the host form runs the bodies host_mul.hip runs.  NORMALISE works on a copy of the records,
// because mul_normalise overwrites them; NORMALISE_RECORDS returns that copy instead of the affine bytes.
namespace {

struct MulStage {
  bool g2 = false, fixed = false, records = false;
  size_t in_stride = 0, out_stride = 0;   // bytes per record of `in` and of `out`
  size_t affine_stride = 0;               // the two normalisation stages: bytes per affine record
};

// false: an unknown group, stage or layout
bool mul_stage_shape(int group, int which, int layout, MulStage* s) {
  if ((group != 1 && group != 2) || which < MSM_AMD_MUL_STAGE_FIXED || which > MSM_AMD_MUL_STAGE_NORMALISE_RECORDS) return false;
  s->g2 = group == 2;
  s->fixed = which == MSM_AMD_MUL_STAGE_FIXED;
  s->records = which == MSM_AMD_MUL_STAGE_NORMALISE_RECORDS;
  if (s->fixed) {
    if (!mul_scalar_layout_known(layout)) return false;
    s->in_stride = 32, s->out_stride = mul_xyzz_bytes(s->g2);
    return true;
  }
  s->affine_stride = point_record_bytes(s->g2, layout, kKindAffine);
  s->in_stride = mul_xyzz_bytes(s->g2);
  s->out_stride = s->records ? s->in_stride : s->affine_stride;
  return s->affine_stride != 0;
}

template <class G>
void mul_stage_host(const MulStage& s, int layout, const uint8_t* in, const void* table, size_t n, uint8_t* out) {
  if (s.fixed) {
    for (size_t i = 0; i < n; ++i)
      G::store_pt((typename G::Pt*)(out + i * s.out_stride),
                  mul_fixed<G>(mul_scalar(layout, in + i * 32), (const typename G::Packed*)table));
    return;
  }
  alignas(16) typename G::Pt recs[kMulNormGroup];
  std::vector<uint8_t> affine(s.records ? kMulNormGroup * s.affine_stride : 0);
  for (size_t first = 0; first < n; first += kMulNormGroup) {   // the groups of mul_normalise_kernel
    const uint32_t m = (uint32_t)std::min<size_t>(kMulNormGroup, n - first);
    std::memcpy(recs, in + first * s.in_stride, m * s.in_stride);
    mul_normalise<G>(recs, m, layout, (uint32_t)s.affine_stride, s.records ? affine.data() : out + first * s.affine_stride);
    if (s.records) std::memcpy(out + first * s.in_stride, recs, m * s.in_stride);
  }
}

}  // namespace

extern "C" {

int msm_amd_test_mul_stage(msm_amd_ctx* ctx, int group, int which, int layout, const void* in, const void* table,
                           size_t n, void* out) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  MulStage s;
  if (!mul_stage_shape(group, which, layout, &s))
    return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_mul_stage: unknown group, stage or layout");
  DeviceCall c;
  c.who = "msm_amd_test_mul_stage";
  CallState& cs = s.g2 ? ctx->g2.calls : ctx->calls;
  c.g2 = s.g2, c.n = n;
  c.all_host(true);
  c.in[0] = in, c.in_bytes[0] = n * s.in_stride;
  c.in[1] = table, c.in_bytes[1] = s.fixed ? mul_table_bytes(s.g2) : 0;
  c.out = out, c.out_bytes = n * s.out_stride;
  if (s.records) c.work[0] = {&cs.xyzz, n * s.affine_stride};   // where the affine bytes of NORMALISE_RECORDS go
  return point_call(
      ctx, c, !in || !out || (s.fixed && !table),
      [&](hipStream_t st, const CallIo& io) -> int {
        if (s.fixed) {
          launch_mul_fixed(st, s.g2, layout, io.in[0], (uint32_t)n, io.in[1], io.out);
        } else if (s.records) {   // the records move to the output buffer and are normalised there
          HIP_TRY(ctx, hipMemcpyAsync(io.out, io.in[0], n * s.in_stride, hipMemcpyDeviceToDevice, st));
          launch_mul_normalise(st, s.g2, io.out, (uint32_t)n, layout, cs.xyzz.p);
        } else {                  // io.in[0] is the staged copy of the caller's records: the kernel may overwrite it
          launch_mul_normalise(st, s.g2, const_cast<void*>(io.in[0]), (uint32_t)n, layout, io.out);
        }
        return MSM_AMD_OK;
      },
      [](const PointCounters&, float) {});
}

int msm_amd_test_mul_stage_host(int group, int which, int layout, const void* in, const void* table, size_t n, void* out) {
  MulStage s;
  if (!mul_stage_shape(group, which, layout, &s) || n > 0xFFFFFFFFull) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  if (!in || !out || (s.fixed && !table)) return MSM_AMD_INPUT_ERROR;
  if (s.g2)
    mul_stage_host<MulG2>(s, layout, (const uint8_t*)in, table, n, (uint8_t*)out);
  else
    mul_stage_host<MulG1>(s, layout, (const uint8_t*)in, table, n, (uint8_t*)out);
  return MSM_AMD_OK;
}

}  // extern "C"

// ---- transform over G1 points (msm_amd_ntt_points, msm_amd_ntt_points_device) ----------------------------------------------
// Through device_call, all on the main stream: the load pass consumes the input into the first packed work array before
// anything is written (so d_out == d_in is an ordinary call), every level runs in chunks of lanes through the XYZZ chunk
// buffer of the mul calls into the other work array, and the last normalisation writes the caller's layout to `out`.
// INVERSE ends with the ladder by n^-1 over the last work array; log_n = 0 sends its one record through that pass with
// the factor 1.
namespace {

// levels: kNttpAllLevels, or 0 .. log_n (msm_amd_test_ntt_points_levels, host buffers): the work array after that many
// levels, affine records of layout_out in network order, no scaling.
int ntt_points_call(msm_amd_ctx* ctx, const msm_amd_ntt_domain* handle, bool host, int direction, int layout_in,
                    const void* in, int layout_out, void* out, float* kernel_ms, uint32_t levels) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = levels != kNttpAllLevels ? "msm_amd_test_ntt_points_levels" : host ? "msm_amd_ntt_points" : "msm_amd_ntt_points_device";
  const std::string& who = c.who;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!ntt_direction_known(direction)) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": direction must be MSM_AMD_NTT_FORWARD or MSM_AMD_NTT_INVERSE");
  if (!nttp_layouts_known(!host, layout_in, layout_out))
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + (host ? ": points in a G1 host layout, output in one of the two affine host layouts (not *_PREPARED / *_TABLES)"
                                                      : ": points in a G1 host layout or *_PREPARED, output in an affine layout or *_PREPARED (not *_TABLES)"));
  const uint32_t prepared = host ? 0u : (uint32_t)kKindPrepared;
  const size_t in_stride = point_record_bytes(false, layout_in, kKindHost | prepared),
               out_stride = point_record_bytes(false, layout_out, kKindAffine | prepared);
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_ntt_domain* dom = find_handle(ctx->live_ntt, handle);
  if (!dom) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": not a transform domain of this ctx");
  const uint32_t log_n = dom->log_n;
  if (levels != kNttpAllLevels && levels > log_n) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": levels must be 0 .. log_n");
  if (!in || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": null pointer");
  const size_t n = (size_t)1 << log_n;
  if (!host) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (a != b && a < b + n * out_stride && b < a + n * in_stride)
      return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": d_out must be d_in itself or disjoint from it");
  }
  const uint32_t run = levels == kNttpAllLevels ? log_n : levels;
  u256 k = u256_zero();
  const bool laddered = levels == kNttpAllLevels && direction == kNttInverse && nttp_n_inv(log_n, &k);
  const bool last_pass = laddered || run == 0;   // the records go through the uniform-scalar pass on their way out
  const uint32_t lanes = (uint32_t)(n / 2), chunk_lanes = nttp_chunk_lanes(log_n, ctx->mul_chunk);
  const size_t chunk = std::min(n, ctx->mul_chunk);   // records per chunk of the last pass
  CallState& s = ctx->calls;
  c.host = host, c.host_in = host ? 1u : 0u, c.kernel_ms = kernel_ms;
  c.in[0] = in, c.in_bytes[0] = n * in_stride;
  c.out = out, c.out_bytes = n * out_stride;
  c.work[0] = {&s.xyzz, std::max<size_t>(2 * (size_t)chunk_lanes, chunk) * mul_xyzz_bytes(false)};
  c.work[1] = {&s.scratch, 2 * n * sizeof(AffPacked)};
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    AffPacked* work[2] = {(AffPacked*)s.scratch.p, (AffPacked*)s.scratch.p + n};
    void* xyzz = s.xyzz.p;
    launch_nttp_load(st, layout_in, io.in[0], log_n, work[0]);
    int cur = 0;
    for (uint32_t level = 1; level <= run; ++level) {
      const bool to_out = level == run && !last_pass;
      for (uint32_t lane0 = 0; lane0 < lanes; lane0 += chunk_lanes) {
        const uint32_t m = std::min(chunk_lanes, lanes - lane0);
        launch_nttp_level(st, work[cur], dom->d_mem, log_n, level, direction, lane0, m, xyzz);
        launch_nttp_normalise(st, xyzz, log_n, level, lane0, m, to_out ? layout_out : kLayoutPrepared,
                              to_out ? io.out : (void*)work[cur ^ 1]);
      }
      cur ^= 1;
    }
    if (last_pass)
      for (size_t first = 0; first < n; first += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - first);
        launch_nttp_scale(st, work[cur], (uint32_t)first, m, laddered, k, xyzz);
        launch_mul_normalise(st, false, xyzz, m, layout_out, (uint8_t*)io.out + first * out_stride);
      }
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_ntt_points(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                       const void* in, int point_layout_out, void* out) {
  return ntt_points_call(ctx, domain, true, direction, point_layout_in, in, point_layout_out, out, nullptr, kNttpAllLevels);
}

int msm_amd_ntt_points_device(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                              const void* d_in, int point_layout_out, void* d_out, float* kernel_ms) {
  return ntt_points_call(ctx, domain, false, direction, point_layout_in, d_in, point_layout_out, d_out, kernel_ms,
                         kNttpAllLevels);
}

int msm_amd_test_ntt_points_levels(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                                   const void* in, uint32_t levels, int point_layout_out, void* out) {
  if (levels == kNttpAllLevels) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_ntt_points_levels: levels must be 0 .. log_n");
  return ntt_points_call(ctx, domain, true, direction, point_layout_in, in, point_layout_out, out, nullptr, levels);
}

}  // extern "C"

// ---- pairings (msm_amd_pairing_product*, msm_amd_final_exponentiation*, msm_amd_test_fq12_op) ------------------------------
// Through device_call, all on the main stream: the Miller kernel writes one partial product per lane into the first work
// array, the fold levels multiply them down between the two work arrays, and the last kernel turns the one value per
// group into its record (and its unit flag).  When the plan leaves the final exponentiation to the host (host buffers,
// fewer groups than the threshold), that kernel only converts, and the host twin finishes the records where the caller
// gets them.
namespace {

int pairing_call(msm_amd_ctx* ctx, bool host, int layout_g1, int layout_g2, const void* g1, const void* g2, size_t n_groups,
                 size_t group_size, uint32_t flags, int gt_layout, void* out, uint8_t* is_one, float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = host ? "msm_amd_pairing_product" : "msm_amd_pairing_product_device";
  if (kernel_ms) *kernel_ms = 0.f;
  const uint32_t prepared = host ? 0u : (uint32_t)kKindPrepared;
  const size_t s1 = point_record_bytes(false, layout_g1, kKindHost | prepared), s2 = point_record_bytes(true, layout_g2, kKindHost | prepared);
  if (s1 == 0 || s2 == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + (host ? ": points in a host layout of their group only (not *_PREPARED / *_TABLES)"
                                                        : ": points in a host layout of their group or *_PREPARED (not *_TABLES)"));
  if (const char* why = pairing_shape_error(n_groups, group_size, flags, gt_layout, is_one != nullptr))
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": " + why);
  if (n_groups == 0) return MSM_AMD_OK;
  const size_t pairs = n_groups * group_size;
  if (!out || (pairs && (!g1 || !g2))) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": null pointer with work to do");
  uint32_t ppl_knob;
  uint64_t final_from;
  bool f_in_lds;
  pairing_knobs(&ppl_knob, &final_from, &f_in_lds);
  const PairingPlan plan = pairing_plan(n_groups, group_size, ppl_knob, final_from);
  const bool miller_only = (flags & MSM_AMD_PAIRING_MILLER_ONLY) != 0;
  const bool host_final = host && !miller_only && !plan.final_on_device;
  const size_t partial_bytes = kPairingPartialWords * sizeof(uint32_t);
  const size_t folded = (plan.lanes_per_group + kPairingFoldRadix - 1) / kPairingFoldRadix;
  CallState& s = ctx->calls;
  c.host = host, c.host_in = host ? 3u : 0u, c.kernel_ms = kernel_ms;
  c.in[0] = g1, c.in_bytes[0] = pairs * s1;
  c.in[1] = g2, c.in_bytes[1] = pairs * s2;
  c.out = out, c.out_bytes = n_groups * (size_t)MSM_AMD_GT_BYTES;
  c.reasons = host_final ? nullptr : is_one, c.n = c.reasons ? n_groups : 0;
  c.work[0] = {&s.xyzz, n_groups * plan.lanes_per_group * partial_bytes};
  c.work[1] = {&s.scratch, plan.fold_levels ? n_groups * folded * partial_bytes : 0};
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int rc = device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
      uint32_t *cur = (uint32_t*)s.xyzz.p, *other = (uint32_t*)s.scratch.p;
      launch_pairing_miller(st, layout_g1, io.in[0], layout_g2, io.in[1], (uint32_t)n_groups, (uint32_t)group_size, plan, f_in_lds, cur);
      for (uint32_t count = plan.lanes_per_group; count > 1; count = (count + kPairingFoldRadix - 1) / kPairingFoldRadix) {
        launch_pairing_fold(st, cur, (uint32_t)n_groups, count, other);
        std::swap(cur, other);
      }
      launch_pairing_final(st, cur, true, (uint32_t)n_groups, miller_only || host_final, gt_layout, io.out, io.reasons);
      return MSM_AMD_OK;
    });
    if (rc) return rc;
  }
  if (host_final) host_final_exponentiation(gt_layout, (const uint8_t*)out, n_groups, 0, (uint8_t*)out, is_one);
  return MSM_AMD_OK;
}

int final_exp_call(msm_amd_ctx* ctx, bool host, int gt_layout, const void* in, size_t n, void* out, uint8_t* is_one,
                   float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = host ? "msm_amd_final_exponentiation" : "msm_amd_final_exponentiation_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (!pairing_gt_layout_known(gt_layout))
    return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": gt_layout must be MSM_AMD_GT_MONT_LE or MSM_AMD_GT_CANON_LE");
  if (n > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": n >= 2^32");
  if (n == 0) return MSM_AMD_OK;
  if (!in || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": null pointer with n > 0");
  uint32_t ppl_knob;
  uint64_t final_from;
  bool f_in_lds;
  pairing_knobs(&ppl_knob, &final_from, &f_in_lds);
  if (host && n < final_from) {
    host_final_exponentiation(gt_layout, (const uint8_t*)in, n, 0, (uint8_t*)out, is_one);
    return MSM_AMD_OK;
  }
  c.host = host, c.host_in = host ? 1u : 0u, c.kernel_ms = kernel_ms;
  c.in[0] = in, c.in_bytes[0] = n * (size_t)MSM_AMD_GT_BYTES;
  c.out = out, c.out_bytes = n * (size_t)MSM_AMD_GT_BYTES;
  c.reasons = is_one, c.n = is_one ? n : 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    launch_pairing_final(st, io.in[0], false, (uint32_t)n, false, gt_layout, io.out, io.reasons);
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_pairing_product(msm_amd_ctx* ctx, int point_layout, int g2_point_layout, const void* g1_points,
                            const void* g2_points, size_t n_groups, size_t group_size, uint32_t flags, int gt_layout,
                            void* out_gt, uint8_t* is_one) {
  return pairing_call(ctx, true, point_layout, g2_point_layout, g1_points, g2_points, n_groups, group_size, flags, gt_layout,
                      out_gt, is_one, nullptr);
}

int msm_amd_pairing_product_device(msm_amd_ctx* ctx, int point_layout, int g2_point_layout, const void* d_g1_points,
                                   const void* d_g2_points, size_t n_groups, size_t group_size, uint32_t flags,
                                   int gt_layout, void* d_out_gt, uint8_t* d_is_one, float* kernel_ms) {
  return pairing_call(ctx, false, point_layout, g2_point_layout, d_g1_points, d_g2_points, n_groups, group_size, flags,
                      gt_layout, d_out_gt, d_is_one, kernel_ms);
}

int msm_amd_final_exponentiation(msm_amd_ctx* ctx, int gt_layout, const void* in, size_t n, void* out, uint8_t* is_one) {
  return final_exp_call(ctx, true, gt_layout, in, n, out, is_one, nullptr);
}

int msm_amd_final_exponentiation_device(msm_amd_ctx* ctx, int gt_layout, const void* d_in, size_t n, void* d_out,
                                        uint8_t* d_is_one, float* kernel_ms) {
  return final_exp_call(ctx, false, gt_layout, d_in, n, d_out, d_is_one, kernel_ms);
}

int msm_amd_test_fq12_ops(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (op < 0 || op > MSM_AMD_FQ12_OP_FINAL_EXP || count > kTestFq12OpsMax)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_fq12_ops: unknown op or more than 2^20 records");
  if (count == 0) return MSM_AMD_OK;
  if (!a || !b || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_fq12_ops: null pointer with count > 0");
  DeviceCall c;
  c.who = "msm_amd_test_fq12_ops";
  const size_t bytes = count * kPairingPartialWords * sizeof(uint32_t);
  c.all_host(true);
  c.host_in = 3u;
  c.in[0] = a, c.in_bytes[0] = bytes;
  c.in[1] = b, c.in_bytes[1] = bytes;
  c.out = out, c.out_bytes = bytes;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    launch_test_fq12_op(st, op, (const uint32_t*)io.in[0], (const uint32_t*)io.in[1], (uint32_t*)io.out, (uint32_t)count);
    return MSM_AMD_OK;
  });
}

int msm_amd_test_fq12_op(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (!a || !b || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_fq12_op: null pointer");
  return msm_amd_test_fq12_ops(ctx, op, a, b, out, 1);
}

}  // extern "C"
