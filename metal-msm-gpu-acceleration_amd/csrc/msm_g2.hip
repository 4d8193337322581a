// ---- BN254 G2 MSM (one blocking call on the main stream) -----------------------------------------------------------
// A client of the G1 instance pipeline of msm_host.hip and of the planner, through msm_driver.h: the G2 launches bound
// into a PointStages, enqueue_instance in the G2 state's own workspace and slot, the bounded wait, the host Horner pass;
// persistent G2 bases and window tables beside it.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <mutex>
#include <string>

#include "launch_g2.h"
#include "msm_driver.h"

namespace {

// The whole G2 MSM of device-resident inputs: one lone instance (enqueue_instance with the G2 launches) in the G2
// state's own workspace and slot on the main stream, a bounded wait and the host Horner pass.  d_points: n records of a
// host layout, a prepared array (MSM_AMD_G2_POINT_PREPARED: no base conversion) or a table handle
// (MSM_AMD_G2_POINT_TABLES: the one-window plan, every digit window adds into one bucket set).  ctx->mu held by the caller.
int run_msm_g2(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars, const void* d_points,
               size_t n, void* out192) {
  G2State& g2 = ctx->g2;
  g2.has_last_plan = false;   // the stage tap reads nothing of a call that failed
  if (n > 0x7FFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "n >= 2^31");
  if (int rc = recover_if_stalled(ctx)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const msm_amd_g2_tables* tb = nullptr;
  if (g2_point_layout == MSM_AMD_G2_POINT_TABLES) {   // d_points is the handle of msm_amd_g2_tables_build*
    tb = find_handle(ctx->live_g2_tables, d_points);
    if (!tb) return fail(ctx, MSM_AMD_INPUT_ERROR, "not a G2 table handle of this ctx");
    if (n != tb->n) return fail(ctx, MSM_AMD_INPUT_ERROR, "n differs from the number of points the tables hold");
  }
  const bool prepared = tb != nullptr || g2_point_layout == MSM_AMD_G2_POINT_PREPARED;
  const WidthBound width = ctx->bound;
  const uint32_t c = tb ? tb->c : (ctx->forced_window ? ctx->forced_window : auto_window_bounded(n, width.width(), true));
  const Plan p = instance_plan(n, c, tb ? tb->W : 0, true, width);
  Workspace& w = g2.ws;
  InstanceSlot& slot = g2.slot;
  PointStages g;
  g.bases_bytes = prepared ? 0 : n * sizeof(Aff2Packed);
  g.internal_bytes = sizeof(PtI2);
  g.ext_bytes = sizeof(Jacobian2);
  g.convert_bases = [&](hipStream_t st) -> int {
    if (!prepared)
      launch_convert_bases_g2(st, d_points, g2_point_layout == MSM_AMD_G2_POINT_ARK_AFFINE, (uint32_t)n,
                              (Aff2Packed*)w.bases29.p);
    return MSM_AMD_OK;
  };
  g.accumulate = [&](hipStream_t st, const SortBuffers& sb, hipEvent_t before, hipEvent_t after) {
    const void* bases = tb ? tb->d_mem : (prepared ? d_points : w.bases29.p);
    (void)hipEventRecord(before, st);
    launch_accumulate_g2(st, p, (const Aff2Packed*)bases, sb, (PtI2*)w.buckets.p, (PtI2*)w.item_partials.p);
    (void)hipEventRecord(after, st);
  };
  g.combine = [&](hipStream_t st, const SortBuffers& sb) { launch_combine_g2(st, p, sb, (PtI2*)w.buckets.p, (PtI2*)w.item_partials.p); };
  g.reduce = [&](hipStream_t st) {
    launch_reduce_g2(st, p, (const PtI2*)w.buckets.p, (const uint32_t*)w.bsize.p, (PtI2*)w.S.p, (PtI2*)w.T.p, (Jacobian2*)w.partial.p);
  };
  if (int rc = enqueue_instance(ctx, w, slot, p, true, scalar_layout, d_scalars, g)) return rc;
  const hipError_t we = wait_event(slot.ev[EV_REDUCE], ctx->wait_timeout_ms);
  if (we == hipErrorNotReady) return wait_timed_out(ctx, slot, "the G2 MSM");
  if (we != hipSuccess) return fail(ctx, MSM_AMD_PIPELINE_ERROR, std::string("G2 MSM: ") + hipGetErrorString(we));
  const auto t0 = std::chrono::steady_clock::now();
  const Jacobian2 res = host_combine_g2((const Jacobian2*)slot.h_partial, p);
  const float final_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (p.bits) {
    const PlanCounters pc = slot.counters();
    if (pc.viol[0]) {
      reap_graveyard(ctx);
      return fail(ctx, MSM_AMD_INPUT_ERROR, width_violation_message(p, pc.viol[0], 1, 0, 1, ~pc.viol[1]));
    }
  }
  std::memcpy(out192, &res, 192);
  ctx->timings = msm_amd_timings{};
  accumulate_timings(ctx, slot, p, final_ms, 1);
  reap_graveyard(ctx);
  g2.last_plan = p;
  g2.has_last_plan = true;
  return MSM_AMD_OK;
}

// the identity result ((R, 0), (R, 0), (0, 0)) of an empty G2 MSM
void g2_identity_out(void* out192) {
  Jacobian2 r{};
  r.x.c0 = Fq::one();
  r.y.c0 = Fq::one();
  std::memcpy(out192, &r, 192);
}

// `device`: the device-resident entry point, which also takes the two device-only layouts (host layouts are the ones
// msm_amd_g2_point_bytes knows)
int g2_args(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
            const void* out192, bool device = false) {
  if (!ctx || !out192) return MSM_AMD_INPUT_ERROR;
  if (!scalar_layout_ok(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  const bool device_only = g2_point_layout == MSM_AMD_G2_POINT_PREPARED || g2_point_layout == MSM_AMD_G2_POINT_TABLES;
  if (msm_amd_g2_point_bytes(g2_point_layout) == 0 && !(device && device_only))
    return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown G2 point layout");
  if (n > 0 && (!scalars || !points)) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer with n > 0");
  return MSM_AMD_OK;
}

// Conversion of a resident G2 point array (a host layout) to Aff2Packed records; ctx->mu held by the caller.
int prepare_bases_g2_locked(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n, void* d_prepared) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");   // a set-up step
  hipStream_t st = ctx->stream;
  launch_convert_bases_g2(st, d_points, g2_point_layout == MSM_AMD_G2_POINT_ARK_AFFINE, (uint32_t)n,
                          (Aff2Packed*)d_prepared);
  HIP_TRY(ctx, hipGetLastError());
  return sync_stream_bounded(ctx, st, __func__);
}

int g2_tables_build_locked(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n, uint32_t window_size,
                           msm_amd_g2_tables** out) {
  // The automatic table window: auto_table_window (G1) balances the W n mixed additions against the 2^(c-1) buckets of
  // the window reduction; the same balance holds on G2 (every term costs the same factor more), so it is the starting
  // point, and the measurement of DESIGN.md section 8 keeps it.
  uint32_t c, W;
  if (int grc = tables_geometry(ctx, n, window_size, auto_table_window(n), &c, &W)) return grc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");   // a set-up step
  return tables_build_tail(ctx, ctx->live_g2_tables, n, c, W, sizeof(Aff2Packed), "G2 ", [&](void* d_tab) {
    launch_build_tables_g2(ctx->stream, d_points, g2_point_layout == MSM_AMD_G2_POINT_ARK_AFFINE, (uint32_t)n, c, W,
                           (Aff2Packed*)d_tab);
  }, out);
}

}  // namespace

extern "C" {

// msm_amd_msm_g2_device and its bounded form (bits = 0: unbounded)
static int msm_g2_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars, const void* d_points,
                         size_t n, uint32_t bits, int sign, void* out192) {
  if (int rc = g2_args(ctx, scalar_layout, g2_point_layout, d_scalars, d_points, n, out192, true)) return rc;
  if (n == 0 && g2_point_layout != MSM_AMD_G2_POINT_TABLES) {   // (a table never holds 0 points: n mismatch below)
    g2_identity_out(out192);
    return MSM_AMD_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  BoundScope scope(ctx, bits, sign);
  return run_msm_g2(ctx, scalar_layout, g2_point_layout, d_scalars, d_points, n, out192);
}

int msm_amd_msm_g2_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars,
                          const void* d_points, size_t n, void* out192) {
  return msm_g2_device(ctx, scalar_layout, g2_point_layout, d_scalars, d_points, n, 0, 0, out192);
}

int msm_amd_msm_g2_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars,
                                  const void* d_points, size_t n, uint32_t bits, int sign, void* out192) {
  if (int rc = bound_args(ctx, __func__, bits, sign)) return rc;
  return msm_g2_device(ctx, scalar_layout, g2_point_layout, d_scalars, d_points, n, bits, sign, out192);
}

int msm_amd_g2_bases_prepare_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                    void* d_prepared) {
  if (!ctx || !d_points || !d_prepared || n == 0 || n > 0x7FFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad g2_bases_prepare arguments");
  if (msm_amd_g2_point_bytes(g2_point_layout) == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad G2 point layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  return prepare_bases_g2_locked(ctx, g2_point_layout, d_points, n, d_prepared);
}

int msm_amd_g2_bases_upload(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, void** d_prepared) {
  if (!ctx || !points || !d_prepared || n == 0 || n > 0x7FFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad g2_bases_upload arguments");
  const size_t pb = msm_amd_g2_point_bytes(g2_point_layout);
  if (pb == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad G2 point layout");
  *d_prepared = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  return upload_and_prepare(
      ctx, ctx->g2.in_points, points, n * pb, n * sizeof(Aff2Packed), "the resident copy of the G2 bases",
      [&](const void* staged, void* d_out) { return prepare_bases_g2_locked(ctx, g2_point_layout, staged, n, d_out); },
      d_prepared);
}

// host scalars -> the G2 state's staging buffer, on the stream the MSM runs on (stream order does the rest)
static int g2_stage_scalars(msm_amd_ctx* ctx, const void* scalars, size_t n) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  if (int rc = ensure(ctx, ctx->g2.in_scalars, n * 32)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->g2.in_scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
  return MSM_AMD_OK;
}

int msm_amd_msm_g2_prepared(msm_amd_ctx* ctx, int scalar_layout, const void* scalars, const void* d_prepared, size_t n,
                            void* out192) {
  if (!ctx || !scalars || !d_prepared || !out192 || n == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad msm_g2_prepared arguments");
  if (!scalar_layout_ok(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int rc = g2_stage_scalars(ctx, scalars, n)) return rc;
  return run_msm_g2(ctx, scalar_layout, MSM_AMD_G2_POINT_PREPARED, ctx->g2.in_scalars.p, d_prepared, n, out192);
}

int msm_amd_g2_tables_build_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                   uint32_t window_size, msm_amd_g2_tables** out) {
  if (!ctx || !d_points || !out || n == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad g2_tables_build arguments");
  *out = nullptr;
  if (msm_amd_g2_point_bytes(g2_point_layout) == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "G2 tables are built from one of the host point layouts");
  std::lock_guard<std::mutex> g(ctx->mu);
  return g2_tables_build_locked(ctx, g2_point_layout, d_points, n, window_size, out);
}

int msm_amd_g2_tables_build(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, uint32_t window_size,
                            msm_amd_g2_tables** out) {
  if (!ctx || !points || !out || n == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad g2_tables_build arguments");
  *out = nullptr;
  const size_t pb = msm_amd_g2_point_bytes(g2_point_layout);
  if (pb == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "G2 tables are built from one of the host point layouts");
  if (n > 0x7FFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "windows * n must stay below 2^31");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure(ctx, ctx->g2.in_points, n * pb)) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->g2.in_points.p, points, n * pb, hipMemcpyHostToDevice));
  return g2_tables_build_locked(ctx, g2_point_layout, ctx->g2.in_points.p, n, window_size, out);
}

int msm_amd_g2_tables_info(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, size_t* n, uint32_t* window_size,
                           uint32_t* num_windows, size_t* device_bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return tables_info(ctx, ctx->live_g2_tables, tables, "not a G2 table handle of this ctx", n,
                     window_size, num_windows, device_bytes);
}

int msm_amd_g2_tables_free(msm_amd_ctx* ctx, msm_amd_g2_tables* tables) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return handle_free(ctx, ctx->live_g2_tables, tables, "not a G2 table handle of this ctx");
}

int msm_amd_msm_g2_tables(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, int scalar_layout, const void* scalars,
                          void* out192) {
  if (!ctx || !tables || !scalars || !out192) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad msm_g2_tables arguments");
  if (!scalar_layout_ok(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  const msm_amd_g2_tables* t = find_handle(ctx->live_g2_tables, tables);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, "not a G2 table handle of this ctx");
  if (int rc = g2_stage_scalars(ctx, scalars, t->n)) return rc;
  return run_msm_g2(ctx, scalar_layout, MSM_AMD_G2_POINT_TABLES, ctx->g2.in_scalars.p, tables, t->n, out192);
}

// msm_amd_msm_g2 and its bounded form (bits = 0: unbounded)
static int msm_g2_host(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars, const void* points,
                       size_t n, uint32_t bits, int sign, void* out192) {
  if (int rc = g2_args(ctx, scalar_layout, g2_point_layout, scalars, points, n, out192)) return rc;
  if (n == 0) {
    g2_identity_out(out192);
    return MSM_AMD_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  BoundScope scope(ctx, bits, sign);
  G2State& g = ctx->g2;
  const size_t pb = n * msm_amd_g2_point_bytes(g2_point_layout);
  if (int rc = g2_stage_scalars(ctx, scalars, n)) return rc;
  if (int rc = ensure(ctx, g.in_points, pb)) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(g.in_points.p, points, pb, hipMemcpyHostToDevice, ctx->stream));
  return run_msm_g2(ctx, scalar_layout, g2_point_layout, g.in_scalars.p, g.in_points.p, n, out192);
}

int msm_amd_msm_g2(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars, const void* points,
                   size_t n, void* out192) {
  return msm_g2_host(ctx, scalar_layout, g2_point_layout, scalars, points, n, 0, 0, out192);
}

int msm_amd_msm_g2_bounded(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars, const void* points,
                           size_t n, uint32_t bits, int sign, void* out192) {
  if (int rc = bound_args(ctx, __func__, bits, sign)) return rc;
  return msm_g2_host(ctx, scalar_layout, g2_point_layout, scalars, points, n, bits, sign, out192);
}

}  // extern "C"
