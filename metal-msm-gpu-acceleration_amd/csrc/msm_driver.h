// What the units of the MSM driver take from each other: msm_host.hip (the ctx and the G1 pipeline), msm_plan.hip (the
// planner), msm_g2.hip (the G2 MSM, a client of the G1 instance pipeline) and calls_stages.hip (the stage entry points
// and the test aids).  Private to csrc/: not installed.  Like the helpers of host_ctx.h these names are in msm_amd::drv
// with hidden visibility; each is defined in the unit its section names.  The list is closed: a name that one unit alone
// uses stays in that unit's anonymous namespace, and the blocking vector calls (calls_points.hip, calls_ntt.hip,
// calls_fr.hip) do not include this header.
#pragma once
#include <functional>

#include "host_ctx.h"

namespace msm_amd {
namespace drv __attribute__((visibility("hidden"))) {

// ---- msm_plan.hip ------------------------------------------------------------------------------------------------------
uint32_t floor_log2(size_t n);
uint32_t auto_window_bounded(size_t n, uint32_t bits, bool lone);
Plan make_reduce_plan(uint32_t lb, uint32_t W);
int tables_geometry(msm_amd_ctx* ctx, size_t n, uint32_t window_size, uint32_t auto_c, uint32_t* c, uint32_t* W);
Plan instance_plan(size_t n, uint32_t c, uint32_t table_windows, bool lone, WidthBound width);
uint32_t auto_table_window(size_t n);

// ---- msm_host.hip ------------------------------------------------------------------------------------------------------
hipError_t wait_event(hipEvent_t ev, uint32_t timeout_ms);
void reap_graveyard(msm_amd_ctx* ctx);
Jacobian iso_to_e(const Jacobian& q);
Jacobian host_combine(const Jacobian* partial, const Plan& p);
int reduce_buffers(msm_amd_ctx* ctx, Workspace& w, const Plan& p, size_t internal_bytes, size_t ext_bytes);
bool scalar_layout_ok(int scalar_layout);

// What the instance body knows of the group it runs (G1 or G2): the record sizes of the point-valued buffers and the
// four launches, bound by the caller to the plan and the workspace of the instance.  Each launch enqueues on the
// stream it is handed.
struct PointStages {
  size_t bases_bytes;      // room the base conversion needs in Workspace::bases29 (0: the bases are resident elsewhere)
  size_t internal_bytes;   // internal point (PtI / PtI2): buckets, item partials, S, T
  size_t ext_bytes;        // external point (Jacobian / Jacobian2): the partial points
  std::function<int(hipStream_t)> convert_bases;   // the caller's points -> packed bases
  // `before` / `after` are recorded directly around the accumulate kernel
  std::function<void(hipStream_t, const SortBuffers&, hipEvent_t before, hipEvent_t after)> accumulate;
  std::function<void(hipStream_t, const SortBuffers&)> combine;
  std::function<void(hipStream_t)> reduce;   // Workspace::buckets, bsize -> partial
};

int enqueue_instance(msm_amd_ctx* ctx, Workspace& w, InstanceSlot& slot, const Plan& p, bool lone, int scalar_layout,
                     const void* d_scalars, const PointStages& g);
void accumulate_timings(msm_amd_ctx* ctx, InstanceSlot& s, const Plan& p, float final_ms, size_t n_inst);
std::string width_violation_message(const Plan& p, size_t records, size_t instances, size_t instance, size_t n_inst,
                                    size_t index);
int wait_timed_out(msm_amd_ctx* ctx, const InstanceSlot& s, const std::string& what, const char* tail = "");
int bound_args(msm_amd_ctx* ctx, const char* who, uint32_t bits, int sign);

// The instances submitted while this lives are planned with `width` (ctx->mu is held by the entry point).
struct BoundScope {
  msm_amd_ctx* ctx;
  BoundScope(msm_amd_ctx* c, uint32_t bits, int sign) : ctx(c) { ctx->bound.bits = bits, ctx->bound.sign = (uint32_t)sign; }
  ~BoundScope() { ctx->bound = WidthBound{}; }
};

// Room for W * n records of record_bytes and handle_build_tail; `group` is "" or "G2 " in messages.
template <class H, class Launch>
int tables_build_tail(msm_amd_ctx* ctx, std::vector<H*>& live, size_t n, uint32_t c, uint32_t W, size_t record_bytes,
                      const std::string& group, Launch&& launch, H** out) {
  if (int rc = handle_build_tail(ctx, live, (size_t)W * n * record_bytes, "the " + group + "window tables",
                                 group + "table build", launch, out)) return rc;
  (*out)->n = n, (*out)->c = c, (*out)->W = W;
  return MSM_AMD_OK;
}

template <class H>
int tables_info(msm_amd_ctx* ctx, const std::vector<H*>& live, const H* tables, const char* not_a_handle, size_t* n,
                uint32_t* window_size, uint32_t* num_windows, size_t* device_bytes) {
  const H* t = find_handle(live, tables);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, not_a_handle);
  if (n) *n = t->n;
  if (window_size) *window_size = t->c;
  if (num_windows) *num_windows = t->W;
  if (device_bytes) *device_bytes = t->bytes;
  return MSM_AMD_OK;
}

// Host points -> `stage` (device scratch) -> a fresh device array of out_bytes that `convert(staged, d_out)` fills and
// waits for with the ctx's bound (prepare_bases_locked and its G2 twin); *d_prepared receives the array.
template <class Convert>
int upload_and_prepare(msm_amd_ctx* ctx, DeviceBuf& stage, const void* points, size_t in_bytes, size_t out_bytes,
                       const char* what, Convert&& convert, void** d_prepared) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure(ctx, stage, in_bytes)) return rc;
  void* d_out = nullptr;
  if (int qrc = quiesce_for_allocation(ctx, what)) return qrc;
  HIP_TRY(ctx, hipMalloc(&d_out, out_bytes));
  hipError_t e = hipMemcpy(stage.p, points, in_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d_out);
    HIP_TRY(ctx, e);
  }
  if (int rc = convert(stage.p, d_out)) {
    // a bounded wait that timed out: the conversion may still be running, and hipFree would wait for the device
    // without bound -- released when the ctx is idle
    if (rc == MSM_AMD_PIPELINE_ERROR) ctx->graveyard.push_back(d_out);
    else (void)hipFree(d_out);
    return rc;
  }
  *d_prepared = d_out;
  return MSM_AMD_OK;
}

}  // namespace drv
}  // namespace msm_amd
