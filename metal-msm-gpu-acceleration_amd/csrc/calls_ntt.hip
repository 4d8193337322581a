// The blocking transform calls over Fr (device_call.h): the domain handles, the transform, the passes and twiddles taps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "device_call.h"

// ---- number-theoretic transform over Fr (msm_amd_ntt_domain_*, msm_amd_ntt, msm_amd_ntt_device) --------------------------
// Through device_call: the passes on the main stream; the host form transforms the staged copy of its input in place.
// Domain handles are validated by membership in ctx->live_ntt, under the lock and before anything is sized by them.
namespace {

// max_passes: kNttAllPasses, or 1 .. the pass count of the plan (msm_amd_test_ntt_passes, host buffers): what the first
// max_passes passes wrote -- short of the plan's count that is the pass buffer, copied over the staged input.
int ntt_call(msm_amd_ctx* ctx, const msm_amd_ntt_domain* handle, bool host, int direction, int scalar_layout,
             const void* shift32, const void* in, void* out, size_t n_vec, float* kernel_ms, uint32_t max_passes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall c;
  c.who = max_passes != kNttAllPasses ? "msm_amd_test_ntt_passes" : host ? "msm_amd_ntt" : "msm_amd_ntt_device";
  const std::string& who = c.who;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!ntt_direction_known(direction)) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": direction must be MSM_AMD_NTT_FORWARD or MSM_AMD_NTT_INVERSE");
  if (!ntt_layout_known(scalar_layout))
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": scalars in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE only");
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_ntt_domain* dom = find_handle(ctx->live_ntt, handle);
  if (!dom) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": not a transform domain of this ctx");
  if (((uint64_t)n_vec >> (32 - dom->log_n)) != 0) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": n_vec * n >= 2^32");
  const uint32_t plan_passes = ntt_plan(dom->log_n, ctx->ntt_tile_log).passes;
  if (max_passes != kNttAllPasses && (max_passes == 0 || max_passes > plan_passes))
    return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": passes must be 1 .. the pass count of the plan");
  const bool stopped = max_passes < plan_passes;   // the last pass does not run
  if (n_vec == 0) return MSM_AMD_OK;
  if (!in || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": null pointer with n_vec > 0");
  u256 g;
  if (!ntt_read_shift(scalar_layout, shift32, &g)) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": the shift is 0 mod r");
  const size_t bytes = (n_vec << dom->log_n) * 32;
  if (!host) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if ((a | b) & 15u) return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": d_in and d_out must be 16-byte aligned");
    if (a != b && a < b + bytes && b < a + bytes)
      return fail(ctx, MSM_AMD_INPUT_ERROR, who + ": d_out must be d_in itself or disjoint from it");
  }
  CallState& s = ctx->calls;
  NttLaunch t{};
  t.tw = dom->d_mem, t.log_n = dom->log_n, t.tile_log = ctx->ntt_tile_log;
  t.direction = direction, t.layout = scalar_layout, t.n_vec = n_vec;
  u256 tab[kNttPowEntries];   // the powers of the shift: host memory in either form, staged in `pow`
  ntt_shift_setup(g, direction, dom->log_n, tab, &t.sc);
  c.host = c.in_place = host, c.host_in = (host ? 1u : 0u) | 2u, c.kernel_ms = kernel_ms;
  c.in[0] = in, c.in_bytes[0] = bytes;
  c.in[1] = tab, c.in_bytes[1] = shift32 ? sizeof tab : 0, c.stage[1] = &s.pow;
  c.out = out, c.out_bytes = bytes;
  c.work[0] = {&s.scratch, plan_passes > 1 ? bytes : 0};
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    t.in = io.in[0], t.out = io.out, t.scratch = s.scratch.p, t.pow_tab = shift32 ? io.in[1] : nullptr;
    launch_ntt(st, t, max_passes);
    if (stopped) HIP_TRY(ctx, hipMemcpyAsync(io.out, s.scratch.p, bytes, hipMemcpyDeviceToDevice, st));
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

int msm_amd_ntt_domain_build(msm_amd_ctx* ctx, int root, uint32_t log_n, msm_amd_ntt_domain** out) {
  if (!ctx || !out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_ntt_domain_build: null pointer");
  *out = nullptr;
  if (!ntt_root_known(root)) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_ntt_domain_build: root must be MSM_AMD_NTT_ROOT_ARK or MSM_AMD_NTT_ROOT_H2C");
  if (log_n > kNttMaxLog) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_ntt_domain_build: log_n must be 0..28");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  const u256 omega = ntt_omega(root, log_n);
  const size_t bytes = std::max<size_t>(32, ((size_t)1 << log_n) / 2 * 32);   // n = 1: no entry, one record of room
  if (int rc = handle_build_tail(ctx, ctx->live_ntt, bytes, "the twiddles of a transform domain", "transform domain build",
                                 [&](void* d_tw) { launch_ntt_twiddles(ctx->stream, omega, log_n, d_tw); }, out))
    return rc;
  (*out)->root = root, (*out)->log_n = log_n, (*out)->omega = omega;
  return MSM_AMD_OK;
}

int msm_amd_ntt_domain_info(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int* root, uint32_t* log_n,
                            size_t* device_bytes, void* omega32) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_ntt_domain* d = find_handle(ctx->live_ntt, domain);
  if (!d) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_ntt_domain_info: not a transform domain of this ctx");
  if (root) *root = d->root;
  if (log_n) *log_n = d->log_n;
  if (device_bytes) *device_bytes = d->bytes;
  if (omega32) std::memcpy(omega32, d->omega.v, 32);
  return MSM_AMD_OK;
}

int msm_amd_ntt_domain_free(msm_amd_ctx* ctx, msm_amd_ntt_domain* domain) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return handle_free(ctx, ctx->live_ntt, domain, "msm_amd_ntt_domain_free: not a transform domain of this ctx");
}

int msm_amd_ntt(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout, const void* shift32,
                const void* in, void* out, size_t n_vec) {
  return ntt_call(ctx, domain, true, direction, scalar_layout, shift32, in, out, n_vec, nullptr, kNttAllPasses);
}

int msm_amd_ntt_device(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout,
                       const void* shift32, const void* d_in, void* d_out, size_t n_vec, float* kernel_ms) {
  return ntt_call(ctx, domain, false, direction, scalar_layout, shift32, d_in, d_out, n_vec, kernel_ms, kNttAllPasses);
}

int msm_amd_test_ntt_passes(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout,
                            const void* shift32, const void* in, void* out, size_t n_vec, uint32_t passes) {
  if (passes == kNttAllPasses) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_ntt_passes: passes must be 1 .. the pass count of the plan");
  return ntt_call(ctx, domain, true, direction, scalar_layout, shift32, in, out, n_vec, nullptr, passes);
}

int msm_amd_test_ntt_twiddles(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, size_t first, size_t count, void* out) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> lk(ctx->mu);
  const msm_amd_ntt_domain* d = find_handle(ctx->live_ntt, domain);
  if (!d) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_ntt_twiddles: not a transform domain of this ctx");
  const size_t entries = ((size_t)1 << d->log_n) / 2;
  if (first > entries || count > entries - first)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_ntt_twiddles: range outside the n/2 entries of the table");
  if (count == 0) return MSM_AMD_OK;
  if (!out) return fail(ctx, MSM_AMD_INPUT_ERROR, "msm_amd_test_ntt_twiddles: null pointer with count > 0");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(out, (const u256*)d->d_mem + first, count * 32, hipMemcpyDeviceToHost, ctx->stream));
  return sync_stream_bounded(ctx, ctx->stream, __func__);
}

}  // extern "C"
