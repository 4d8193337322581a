// The reference-shaped stage entry points (prepare / sort / accumulate / reduce / final accumulation on the reference's
// wire layout) and the test aids of both groups: single-op and raw-limb ops with their host twins, the hold kernel, the
// stage taps, the workspace poisoning.  The blocking ones that fit it run on device_call (device_call.h) like the vector
// calls; msm_amd_bucket_wise_accumulation and msm_amd_sum_reduction use workspace 0 and more work buffers than a
// DeviceCall names, and enqueue by hand.  What they take from the MSM driver is declared in msm_driver.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "device_call.h"
#include "msm_driver.h"
#include "launch_g2.h"
#include "launch_compress.h"
#include "host_fq64.h"
#include "test_ops.hip.h"
#include "test_ops_g2.hip.h"

namespace {

// ---- host-side big-endian-limb helpers (reference wire layout) ----------------------------------
u256 be32_to_u256(const uint32_t* l) {
  u256 r;
  for (int i = 0; i < 8; ++i) r.v[i] = l[7 - i];
  return r;
}
void u256_to_be32(const u256& a, uint32_t* l) {
  for (int i = 0; i < 8; ++i) l[i] = a.v[7 - i];
}
Jacobian be32_to_jac(const uint32_t* l) {
  Jacobian r;
  r.x = be32_to_u256(l);
  r.y = be32_to_u256(l + 8);
  r.z = be32_to_u256(l + 16);
  return r;
}
void jac_to_be32(const Jacobian& p, uint32_t* l) {
  u256_to_be32(p.x, l);
  u256_to_be32(p.y, l + 8);
  u256_to_be32(p.z, l + 16);
}

// The pair sort of msm_amd_sort_buckets_indices (host pairs: sorted in the staging, copied back from there) and of
// msm_amd_sort_pairs_device (device pairs, timed).  The radix passes go back and forth between the pairs and scratch_b;
// after an odd number of them the result sits in the scratch buffer and is copied over the pairs, inside the timed span.
int sort_pairs_call(msm_amd_ctx* ctx, const char* who, bool host, void* pairs, size_t n_pairs, uint32_t key_bits,
                    float* kernel_ms) {
  const uint32_t tiles = (uint32_t)((n_pairs + kRadixTile - 1) / kRadixTile);
  DeviceCall c;
  c.who = who;
  c.host = c.in_place = host;
  c.host_in = host ? 1u : 0u;
  c.kernel_ms = kernel_ms;
  c.in[0] = pairs, c.in_bytes[0] = n_pairs * 8;
  c.out = pairs, c.out_bytes = n_pairs * 8;
  c.work[0] = {&ctx->scratch_b, n_pairs * 8};
  c.work[1] = {&ctx->scratch_c, ((size_t)tiles + 1) * 256 * 4};   // the tile histograms
  std::lock_guard<std::mutex> g(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    uint2* src = nullptr;
    launch_radix_sort_pairs(st, (uint2*)io.out, (uint2*)ctx->scratch_b.p, n_pairs, (uint32_t*)ctx->scratch_c.p, &src,
                            key_bits);
    HIP_TRY(ctx, hipGetLastError());
    if (src != (uint2*)io.out)   // odd number of passes: the result sits in the scratch buffer
      HIP_TRY(ctx, hipMemcpyAsync(io.out, src, n_pairs * 8, hipMemcpyDeviceToDevice, st));
    return MSM_AMD_OK;
  });
}

}  // namespace

extern "C" {

// ---- per-stage entry points ------------------------------------------------------------------------
int msm_amd_prepare_buckets_indices(msm_amd_ctx* ctx, const uint32_t* scalars_be32, size_t n, uint32_t window_size,
                                    uint32_t num_windows, uint32_t* pairs_out) {
  if (!ctx || !scalars_be32 || !pairs_out || n == 0 || window_size == 0 || window_size > 32 || num_windows == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad prepare_buckets_indices arguments");
  DeviceCall c;
  c.who = __func__;
  c.all_host(true);
  c.host_in = 1u;
  c.in[0] = scalars_be32, c.in_bytes[0] = n * 32;
  c.out = pairs_out, c.out_bytes = n * num_windows * 8;
  c.work[0] = {&ctx->scratch_b, n * 32};   // the scalars as LE u256
  std::lock_guard<std::mutex> g(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    launch_be32_to_le(st, (const uint32_t*)io.in[0], n, (uint32_t*)ctx->scratch_b.p);
    launch_ref_prepare(st, (const u256*)ctx->scratch_b.p, (uint32_t)n, window_size, num_windows, (uint2*)io.out);
    return MSM_AMD_OK;
  });
}

int msm_amd_sort_buckets_indices(msm_amd_ctx* ctx, uint32_t* pairs, size_t n_pairs) {
  if (!ctx || !pairs) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer");
  if (n_pairs == 0) return MSM_AMD_OK;
  if (n_pairs > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "too many pairs");
  return sort_pairs_call(ctx, __func__, true, pairs, n_pairs, 32, nullptr);
}

int msm_amd_sort_pairs_device(msm_amd_ctx* ctx, void* d_pairs, size_t n_pairs, uint32_t key_bits, float* kernel_ms) {
  if (!ctx || !d_pairs || key_bits == 0 || key_bits > 32) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad sort arguments");
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_pairs == 0) return MSM_AMD_OK;
  if (n_pairs > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "too many pairs");
  return sort_pairs_call(ctx, __func__, false, d_pairs, n_pairs, key_bits, kernel_ms);
}

int msm_amd_bucket_wise_accumulation(msm_amd_ctx* ctx, const uint32_t* sorted_pairs, size_t n_pairs,
                                     const uint32_t* points_be32, size_t n_points, uint32_t total_buckets,
                                     uint32_t* buckets_out) {
  if (!ctx || !sorted_pairs || !points_be32 || !buckets_out || n_points == 0 || total_buckets == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad bucket_wise_accumulation arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx))   // workspace 0 may belong to an MSM between submit_batch_device and wait_batch
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");
  hipStream_t st = ctx->stream;
  int rc;
  const size_t pts_bytes = n_points * 96, bkt_bytes = (size_t)total_buckets * 96;
  if ((rc = ensure(ctx, ctx->scratch_a, std::max(pts_bytes, bkt_bytes)))) return rc;   // BE32 staging
  if ((rc = ensure(ctx, ctx->scratch_b, pts_bytes))) return rc;                        // points LE
  if ((rc = ensure(ctx, ctx->scratch_c, std::max<size_t>(n_pairs * 8, 8)))) return rc;
  if ((rc = ensure(ctx, ctx->ws[0].buckets, bkt_bytes))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, points_be32, pts_bytes, hipMemcpyHostToDevice, st));
  launch_be32_to_le(st, (const uint32_t*)ctx->scratch_a.p, n_points * 3, (uint32_t*)ctx->scratch_b.p);
  HIP_TRY(ctx, hipMemsetAsync(ctx->ws[0].buckets.p, 0, bkt_bytes, st));   // Appendix B item 8: explicit zero fill
  if (n_pairs) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_c.p, sorted_pairs, n_pairs * 8, hipMemcpyHostToDevice, st));
    launch_ref_accumulate(st, (const uint2*)ctx->scratch_c.p, n_pairs, (const Jacobian*)ctx->scratch_b.p,
                          (uint32_t)n_points, total_buckets, (Jacobian*)ctx->ws[0].buckets.p);
  }
  // LE -> BE32 is the same limb reversal
  launch_be32_to_le(st, (const uint32_t*)ctx->ws[0].buckets.p, (size_t)total_buckets * 3, (uint32_t*)ctx->scratch_a.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(buckets_out, ctx->scratch_a.p, bkt_bytes, hipMemcpyDeviceToHost, st));
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_sum_reduction(msm_amd_ctx* ctx, const uint32_t* buckets_be32, uint32_t buckets_size,
                          uint32_t num_windows, uint32_t* res_out) {
  if (!ctx || !buckets_be32 || !res_out || buckets_size == 0 || num_windows == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad sum_reduction arguments");
  // production layout: nb = 2^lb >= buckets_size slots per window, slot i carries weight i + 1
  uint32_t c = kSegLog;
  while ((1u << c) < buckets_size) ++c;
  if (c > 24) return fail(ctx, MSM_AMD_INPUT_ERROR, "buckets_size too large");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx))   // workspace 0 may belong to an MSM between submit_batch_device and wait_batch
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");
  hipStream_t st = ctx->stream;
  const Plan p = make_reduce_plan(c, num_windows);
  int rc;
  const size_t in_bytes = (size_t)buckets_size * num_windows * 96;
  if ((rc = ensure(ctx, ctx->scratch_a, in_bytes))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, in_bytes))) return rc;
  Workspace& ws = ctx->ws[0];
  if ((rc = ensure(ctx, ws.buckets, p.total_buckets * sizeof(PtI)))) return rc;
  if ((rc = reduce_buffers(ctx, ws, p, sizeof(PtI), sizeof(Jacobian)))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, buckets_be32, in_bytes, hipMemcpyHostToDevice, st));
  const size_t words = (size_t)buckets_size * num_windows * 3;
  launch_be32_to_le(st, (const uint32_t*)ctx->scratch_a.p, words, (uint32_t*)ctx->scratch_b.p);
  launch_pad_buckets(st, (const Jacobian*)ctx->scratch_b.p, buckets_size, p.W, p.lb, (PtI*)ws.buckets.p);
  // every bucket holds a valid point: no bucket_size
  launch_reduce(st, p, (const PtI*)ws.buckets.p, nullptr, (PtI*)ws.S.p, (PtI*)ws.T.p, (Jacobian*)ws.partial.p);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<Jacobian> partial(p.partial_count);
  HIP_TRY(ctx, hipMemcpyAsync(partial.data(), ws.partial.p, p.partial_count * sizeof(Jacobian), hipMemcpyDeviceToHost, st));
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  // per-window value: reuse the fused Horner with a single window
  Plan one = p;
  one.W = 1;
  for (uint32_t w = 0; w < num_windows; ++w) {
    const Jacobian r = host_combine(partial.data() + (size_t)w * (p.lb + 1), one);
    jac_to_be32(r, res_out + (size_t)w * 24);
  }
  return MSM_AMD_OK;
}

int msm_amd_sum_points(const void* points96, size_t count, void* out96) {
  if ((!points96 && count) || !out96) return MSM_AMD_INPUT_ERROR;
  h64::Jac acc = h64::identity();
  for (size_t i = 0; i < count; ++i) {
    h64::Jac p;
    std::memcpy(&p, (const uint8_t*)points96 + i * 96, 96);
    acc = h64::jadd(acc, p);
  }
  const h64::Jac res = h64::normalise(acc);
  std::memcpy(out96, &res, 96);
  return MSM_AMD_OK;
}

int msm_amd_final_accumulation(const uint32_t* res_be32, uint32_t num_windows, uint32_t window_size,
                               uint32_t* point_out) {
  if (!res_be32 || !point_out || num_windows == 0) return MSM_AMD_INPUT_ERROR;
  h64::Jac acc = h64::identity();   // same formulas as jac_double / jac_add: identical coordinates, not only the same point
  for (int w = (int)num_windows - 1; w >= 0; --w) {
    for (uint32_t i = 0; i < window_size; ++i) acc = h64::jdouble(acc);
    acc = h64::jadd(acc, h64::load(be32_to_jac(res_be32 + (size_t)w * 24)));
  }
  jac_to_be32(h64::store(acc), point_out);
  return MSM_AMD_OK;
}

// Layout helper for the test-op entry points: limb reversal between the BE32 wire format and LE u256.
static void test_op_widths(int op, size_t* wa, size_t* wb) {
  const bool pt = test_op_is_point(op);
  *wa = pt ? 3 : 1;
  *wb = (op == MSM_AMD_OP_EC_MUL) ? 1 : *wa;
}

int msm_amd_test_op(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!ctx || !a || !b || !out || count == 0 || op < 0 || op > kTestOpMax ||
      (op >= MSM_AMD_OP_H64_FP_MUL && op <= MSM_AMD_OP_H64_EC_DBL))   // (host-only ops 37, 38 are above kTestOpMax)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_op arguments");
  size_t wa, wb;
  test_op_widths(op, &wa, &wb);
  const size_t wo = wa;
  std::vector<uint32_t> la(count * wa * 8), lb(count * wb * 8), lo(count * wo * 8);
  for (size_t i = 0; i < count * wa; ++i)
    for (int l = 0; l < 8; ++l) la[i * 8 + l] = a[i * 8 + 7 - l];
  for (size_t i = 0; i < count * wb; ++i)
    for (int l = 0; l < 8; ++l) lb[i * 8 + l] = b[i * 8 + 7 - l];
  DeviceCall c;
  c.who = __func__;
  c.all_host(true);
  c.host_in = 3u;
  c.in[0] = la.data(), c.in_bytes[0] = la.size() * 4;
  c.in[1] = lb.data(), c.in_bytes[1] = lb.size() * 4;
  c.out = lo.data(), c.out_bytes = lo.size() * 4;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int rc = device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
        launch_test_op(st, op, (const u256*)io.in[0], (const u256*)io.in[1], (u256*)io.out, (uint32_t)count);
        return MSM_AMD_OK;
      }))
    return rc;
  for (size_t i = 0; i < count * wo; ++i)
    for (int l = 0; l < 8; ++l) out[i * 8 + l] = lo[i * 8 + 7 - l];
  return MSM_AMD_OK;
}

// ops 27..31, 37, 38 exist on the host only: the 4 x 64-bit arithmetic of the CPU tail (host_fq64.h)
static bool host64_test_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  const bool inverse = op == MSM_AMD_OP_H64_FP_INV || op == MSM_AMD_OP_H64_FP_INV_FERMAT;
  if ((op < MSM_AMD_OP_H64_FP_MUL || op > MSM_AMD_OP_H64_EC_DBL) && !inverse) return false;
  const bool pt = op == MSM_AMD_OP_H64_EC_ADD || op == MSM_AMD_OP_H64_EC_DBL;
  for (size_t t = 0; t < count; ++t) {
    if (!pt) {
      const u256 xa = be32_to_u256(a + t * 8), xb = be32_to_u256(b + t * 8);
      h64::Fe x, y, r;
      std::memcpy(&x, &xa, 32);
      std::memcpy(&y, &xb, 32);
      if (inverse) r = op == MSM_AMD_OP_H64_FP_INV ? h64::inv(x) : h64::inv_fermat(x);
      else r = op == MSM_AMD_OP_H64_FP_MUL ? h64::mul(x, y) : (op == MSM_AMD_OP_H64_FP_ADD ? h64::add(x, y) : h64::sub(x, y));
      u256 ro;
      std::memcpy(&ro, &r, 32);
      u256_to_be32(ro, out + t * 8);
    } else {
      const h64::Jac p = h64::load(be32_to_jac(a + t * 24)), q = h64::load(be32_to_jac(b + t * 24));
      jac_to_be32(h64::store(op == MSM_AMD_OP_H64_EC_ADD ? h64::jadd(p, q) : h64::jdouble(p)), out + t * 24);
    }
  }
  return true;
}

int msm_amd_test_op_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!a || !b || !out || count == 0 || op < 0) return MSM_AMD_INPUT_ERROR;
  if (host64_test_op(op, a, b, out, count)) return MSM_AMD_OK;
  if (op > kTestOpMax) return MSM_AMD_INPUT_ERROR;
  size_t wa, wb;
  test_op_widths(op, &wa, &wb);
  const size_t wo = wa;
  // the op bodies index points as 3 consecutive u256 per element, scalars of EC_MUL as 1 per element
  std::vector<u256> la(count * wa), lb(count * std::max(wb, wa)), lo(count * wo);
  for (size_t i = 0; i < count * wa; ++i) la[i] = be32_to_u256(a + i * 8);
  for (size_t i = 0; i < count * wb; ++i) lb[i] = be32_to_u256(b + i * 8);
  for (size_t t = 0; t < count; ++t) run_test_op(op, la.data(), lb.data(), lo.data(), (uint32_t)t);
  for (size_t i = 0; i < count * wo; ++i) u256_to_be32(lo[i], out + i * 8);
  return MSM_AMD_OK;
}

// Raw-limb test ops: the internal limbs pass through unchanged (no from_ext, no reversal, no normalisation).
static bool test_op_raw_args(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  return a && b && out && count > 0 && count <= (1u << 24) && op >= 0 &&
         (op < kRawOpCount || (op >= kRawWideFirst && op < kRawWideFirst + kRawWideCount) || op == MSM_AMD_RAW_FE_SQRT ||
          op == MSM_AMD_RAW_BASES_IN_PLACE || (op >= kRawFoldFirst && op < kRawFoldFirst + kRawFoldCount));
}

int msm_amd_test_op_raw(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!ctx || !test_op_raw_args(op, a, b, out, count)) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_op_raw arguments");
  DeviceCall c;
  c.who = __func__;
  c.all_host(true);
  c.host_in = 3u;
  c.in[0] = a, c.in[1] = b, c.in_bytes[0] = c.in_bytes[1] = count * kRawInWords * 4;
  c.out = out, c.out_bytes = count * kRawOutWords * 4;
  std::lock_guard<std::mutex> g(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    if (op == MSM_AMD_RAW_FE_SQRT)   // the root ladder has a kernel of its own (k_compress.hip)
      launch_sqrt_raw(st, false, (const uint32_t*)io.in[0], (uint32_t*)io.out, (uint32_t)count);
    else
      launch_test_op_raw(st, op, (const uint32_t*)io.in[0], (const uint32_t*)io.in[1], (uint32_t*)io.out, (uint32_t)count);
    return MSM_AMD_OK;
  });
}

int msm_amd_test_op_raw_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!test_op_raw_args(op, a, b, out, count)) return MSM_AMD_INPUT_ERROR;
  if (op == MSM_AMD_RAW_FE_SQRT) {
    for (size_t t = 0; t < count; ++t) raw_sqrt_fq(a + t * kRawInWords, out + t * kRawOutWords);
    return MSM_AMD_OK;
  }
  for (size_t t = 0; t < count; ++t) run_test_op_raw(op, a, b, out, (uint32_t)t);
  return MSM_AMD_OK;
}

// Test aid: occupy the ctx's main stream for at most max_ms (<= 5000) or until msm_amd_test_release -- what a stalled
// device looks like to the host waits.  The kernel has its own time bound, so nothing can stay blocked.
int msm_amd_test_hold(msm_amd_ctx* ctx, uint32_t max_ms, void** handle) {
  if (!ctx || !handle || max_ms == 0 || max_ms > 5000) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_hold arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t* flag = nullptr;
  HIP_TRY(ctx, hipHostMalloc((void**)&flag, 64, hipHostMallocDefault));
  *flag = 0;
  launch_hold(ctx->stream, flag, (uint64_t)max_ms * 100000ull);   // wall_clock64 ticks at 100 MHz
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)hipHostFree(flag);
    HIP_TRY(ctx, e);
  }
  *handle = flag;
  return MSM_AMD_OK;
}

int msm_amd_test_release(msm_amd_ctx* ctx, void* handle) {
  if (!ctx || !handle) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  *(volatile uint32_t*)handle = 1u;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // bounded by the kernel's own limit
  HIP_TRY(ctx, hipHostFree(handle));
  return MSM_AMD_OK;
}

// Stage tap (test aid): what the last instance batch left in its workspaces.  Nothing here runs inside enqueue_msm;
// it reads the host record of the batch (plans, workspace indices, the plan counters copied behind the partial points)
// and copies device buffers after the wait, so the pipeline under test is exactly the shipped one.
static int tap_batch(msm_amd_ctx* ctx, uint32_t j, const Batch** out) {
  if (ctx->last_waited < 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "stage tap: no batch has been waited for");
  const Batch& B = ctx->batches[ctx->last_waited];
  if (B.active || B.n_inst > (size_t)kWorkspaces || B.ws_index.size() != B.n_inst)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "stage tap: the last batch had more instances than the ctx has workspaces");
  if (j >= B.n_inst) return fail(ctx, MSM_AMD_INPUT_ERROR, "stage tap: no such instance in the last batch");
  *out = &B;
  return MSM_AMD_OK;
}

// The MSM_AMD_TP_* words of one instance (G1: instance j of a batch; G2: the last run_msm_g2)
static void tap_plan_words(const Plan& p, const PlanCounters& pc, bool lone, uint32_t instances, uint32_t workspace,
                           uint32_t* out) {
  uint32_t v[MSM_AMD_TEST_PLAN_WORDS] = {};
  v[MSM_AMD_TP_C] = p.c;
  v[MSM_AMD_TP_W] = p.W;
  v[MSM_AMD_TP_W_DIGITS] = p.W_digits;
  v[MSM_AMD_TP_N] = p.n;
  v[MSM_AMD_TP_N_SCALARS] = p.n_scalars;
  v[MSM_AMD_TP_LB] = p.lb;
  v[MSM_AMD_TP_NB] = p.nb;
  v[MSM_AMD_TP_CH] = p.CH;
  v[MSM_AMD_TP_HB] = p.hb;
  v[MSM_AMD_TP_MB] = p.mb;
  v[MSM_AMD_TP_FB] = p.fb;
  v[MSM_AMD_TP_Q] = p.Q;
  v[MSM_AMD_TP_TILED] = p.tiled;
  v[MSM_AMD_TP_BALLOT] = p.ballot;
  v[MSM_AMD_TP_WIDE_DIGITS] = p.wide_digits ? 1u : 0u;
  v[MSM_AMD_TP_LONE] = lone ? 1u : 0u;
  v[MSM_AMD_TP_TOTAL_ITEMS] = pc.total_items;
  v[MSM_AMD_TP_MULTI_COUNT] = pc.multi_count;
  v[MSM_AMD_TP_DEFERRED] = pc.pad[0];
  v[MSM_AMD_TP_RED_GROUP] = p.red_group;
  v[MSM_AMD_TP_RB_THREADS] = p.rb_threads;
  v[MSM_AMD_TP_INSTANCES] = instances;
  v[MSM_AMD_TP_WORKSPACE] = workspace;
  v[MSM_AMD_TP_FRONT_THREADS] = p.front_threads;
  v[MSM_AMD_TP_FUSED_FRONT] = p.fused_front ? 1u : 0u;
  v[MSM_AMD_TP_PACKED] = p.packed ? 1u : 0u;
  std::memcpy(out, v, sizeof v);
}

int msm_amd_test_last_plan(msm_amd_ctx* ctx, uint32_t j, uint32_t* out, size_t count) {
  if (!ctx || !out || count < MSM_AMD_TEST_PLAN_WORDS) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_last_plan arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const Batch* B = nullptr;
  if (int rc = tap_batch(ctx, j, &B)) return rc;
  tap_plan_words(B->plans[j], B->slots[j].counters(), B->lone, (uint32_t)B->n_inst, (uint32_t)B->ws_index[j], out);
  return MSM_AMD_OK;
}

// The point-valued buffers of a group and how one record of each leaves through the tap
struct TapPoints {
  const DeviceBuf* buckets;   // [W][nb] internal points
  const DeviceBuf* partial;   // [W][lb + 1] external points
  size_t bucket_bytes, partial_bytes, out_bytes;   // record sizes: internal point, external point, tap output
  // on_iso: the tapped plan ran on E' (Plan::on_iso) and the record is mapped back to E on its way out
  void (*bucket_out)(const uint8_t* rec, uint8_t* out, bool on_iso);
  void (*partial_out)(const uint8_t* rec, uint8_t* out, bool on_iso);
};

// One buffer of a finished call: `w` holds the index and count buffers (the same formats for G1 and G2), `pts` the
// point-valued ones.  ctx->mu held by the caller.
static int tap_stage_copy(msm_amd_ctx* ctx, const Workspace& w, const Plan& p, const PlanCounters& pc,
                          const TapPoints& pts, int which, void* out, size_t* bytes) {
  const DeviceBuf* src = nullptr;
  size_t dev_bytes = 0, records = 0;
  switch (which) {
    case MSM_AMD_STAGE_DIGITS:
      src = &w.digits;
      dev_bytes = (size_t)p.W_digits * p.n_scalars * (p.wide_digits ? 4 : 2);
      break;
    case MSM_AMD_STAGE_SORTED: src = &w.sorted; dev_bytes = (size_t)p.W * p.n * 4; break;
    case MSM_AMD_STAGE_BUCKET_SIZE: src = &w.bsize; dev_bytes = p.total_buckets * 4; break;
    case MSM_AMD_STAGE_BUCKET_START: src = &w.bstart; dev_bytes = p.total_buckets * 4; break;
    case MSM_AMD_STAGE_ITEM_START: src = &w.istart; dev_bytes = p.total_buckets * 4; break;
    case MSM_AMD_STAGE_WIN_ITEMS: src = &w.win_items; dev_bytes = (size_t)p.W * 4; break;
    case MSM_AMD_STAGE_ORDER: src = &w.order; dev_bytes = (size_t)pc.total_items * 8; break;
    case MSM_AMD_STAGE_MULTI_LIST: src = &w.multi_list; dev_bytes = (size_t)pc.multi_count * 4; break;
    case MSM_AMD_STAGE_BUCKETS:
      src = pts.buckets;
      records = p.total_buckets;
      dev_bytes = records * pts.bucket_bytes;
      break;
    case MSM_AMD_STAGE_PARTIAL:
      src = pts.partial;
      records = p.partial_count;
      dev_bytes = records * pts.partial_bytes;
      break;
    default: return fail(ctx, MSM_AMD_INPUT_ERROR, "test_stage_copy: unknown buffer");
  }
  const bool points = which == MSM_AMD_STAGE_BUCKETS || which == MSM_AMD_STAGE_PARTIAL;
  const size_t out_bytes = points ? records * pts.out_bytes : dev_bytes;
  if (!out) {   // size query
    *bytes = out_bytes;
    return MSM_AMD_OK;
  }
  if (*bytes != out_bytes)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "test_stage_copy: the buffer holds " + std::to_string(out_bytes) + " bytes");
  if (dev_bytes > src->cap) return fail(ctx, MSM_AMD_INPUT_ERROR, "test_stage_copy: buffer smaller than the plan");
  if (dev_bytes == 0) return MSM_AMD_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint8_t> h(dev_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(h.data(), src->p, dev_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = sync_stream_bounded(ctx, ctx->stream, __func__)) return rc;
  if (!points) {
    std::memcpy(out, h.data(), dev_bytes);
    return MSM_AMD_OK;
  }
  const bool bk = which == MSM_AMD_STAGE_BUCKETS;
  const size_t rec = bk ? pts.bucket_bytes : pts.partial_bytes;
  for (size_t i = 0; i < records; ++i)
    (bk ? pts.bucket_out : pts.partial_out)(h.data() + i * rec, (uint8_t*)out + i * pts.out_bytes, p.on_iso);
  return MSM_AMD_OK;
}

// G1 point buffers leave in the wire layout of the stage entry points: Jacobian, 3 x 8 u32 most significant first
static void tap_g1_bucket(const uint8_t* rec, uint8_t* out, bool on_iso) {
  PtI q;
  std::memcpy(&q, rec, sizeof q);
  const Jacobian j = pti_to_ext(q);
  jac_to_be32(on_iso ? iso_to_e(j) : j, (uint32_t*)out);
}
static void tap_g1_partial(const uint8_t* rec, uint8_t* out, bool on_iso) {
  Jacobian q;
  std::memcpy(&q, rec, sizeof q);
  jac_to_be32(on_iso ? iso_to_e(q) : q, (uint32_t*)out);
}

int msm_amd_test_stage_copy(msm_amd_ctx* ctx, uint32_t j, int which, void* out, size_t* bytes) {
  if (!ctx || !bytes) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_stage_copy arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const Batch* B = nullptr;
  if (int rc = tap_batch(ctx, j, &B)) return rc;
  const Workspace& w = ctx->ws[B->ws_index[j]];
  const TapPoints pts = {&w.buckets, &w.partial, sizeof(PtI), sizeof(Jacobian), 96, tap_g1_bucket, tap_g1_partial};
  return tap_stage_copy(ctx, w, B->plans[j], B->slots[j].counters(), pts, which, out, bytes);
}

// Point-valued workspace buffers only: a poisoned index or count could make a kernel gather from wild addresses, a
// poisoned point can only make a result wrong.
int msm_amd_test_fill_workspaces(msm_amd_ctx* ctx, uint8_t byte) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  if (int rc = recover_if_stalled(ctx)) return rc;
  for (const Batch& b : ctx->batches)
    if (b.active) return fail(ctx, MSM_AMD_INPUT_ERROR, "test_fill_workspaces: a batch is in flight");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "test_fill_workspaces: device busy");
  Workspace* all[kWorkspaces + 1];
  for (int k = 0; k < kWorkspaces; ++k) all[k] = &ctx->ws[k];
  all[kWorkspaces] = &ctx->g2.ws;
  for (Workspace* w : all)
    for (DeviceBuf* b : {&w->buckets, &w->item_partials, &w->S, &w->T, &w->partial})
      if (b->p && b->cap) HIP_TRY(ctx, hipMemsetAsync(b->p, byte, b->cap, ctx->stream));
  for (CallState* cs : {&ctx->calls, &ctx->g2.calls})   // staging and work buffers of the vector calls; never their 64-byte record
    for (DeviceBuf* b : cs->scratch_bufs())
      if (b->p && b->cap) HIP_TRY(ctx, hipMemsetAsync(b->p, byte, b->cap, ctx->stream));
  return sync_stream_bounded(ctx, ctx->stream, __func__);
}

int msm_amd_test_g2_tables_read(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, uint32_t w, size_t first,
                                size_t count, void* out) {
  if (!ctx || !out || count == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad g2_tables_read arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  const msm_amd_g2_tables* t = find_handle(ctx->live_g2_tables, tables);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, "not a G2 table handle of this ctx");
  if (w >= t->W || first >= t->n || count > t->n - first)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "window or point range outside the table");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<Aff2Packed> rec(count);
  HIP_TRY(ctx, hipMemcpyAsync(rec.data(), (const Aff2Packed*)t->d_mem + (size_t)w * t->n + first,
                              count * sizeof(Aff2Packed), hipMemcpyDeviceToHost, ctx->stream));
  if (int rc = sync_stream_bounded(ctx, ctx->stream, __func__)) return rc;
  for (size_t i = 0; i < count; ++i) {
    const Affine2 e = aff2packed_to_ext(rec[i]);
    std::memcpy((uint8_t*)out + i * 128, &e, 128);
  }
  return MSM_AMD_OK;
}

// Stage tap of the G2 MSM (test aid): plan, plan counters (behind the partial points in the G2 slot, as for a G1
// instance) and buffers of the last run_msm_g2, read after the call.
static const char* const kNoG2Plan = "G2 stage tap: no G2 MSM of this ctx has succeeded last";

// G2 point buffers leave in the result form of msm_amd_msm_g2 (192 B Jacobian, Montgomery LE; identity: z all zero)
static void tap_g2_bucket(const uint8_t* rec, uint8_t* out, bool) {
  PtI2 q;
  std::memcpy(&q, rec, sizeof q);
  const Jacobian2 e = pt2_to_ext(q);
  std::memcpy(out, &e, sizeof e);
}
static void tap_g2_partial(const uint8_t* rec, uint8_t* out, bool) { std::memcpy(out, rec, sizeof(Jacobian2)); }

int msm_amd_test_g2_last_plan(msm_amd_ctx* ctx, uint32_t* out, size_t count) {
  if (!ctx || !out || count < MSM_AMD_TEST_PLAN_WORDS)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_g2_last_plan arguments");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->g2.has_last_plan) return fail(ctx, MSM_AMD_INPUT_ERROR, kNoG2Plan);
  tap_plan_words(ctx->g2.last_plan, ctx->g2.slot.counters(), true, 1, 0, out);
  return MSM_AMD_OK;
}

int msm_amd_test_g2_stage_copy(msm_amd_ctx* ctx, int which, void* out, size_t* bytes) {
  if (!ctx || !bytes) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_g2_stage_copy arguments");
  std::lock_guard<std::mutex> lk(ctx->mu);
  const G2State& g = ctx->g2;
  if (!g.has_last_plan) return fail(ctx, MSM_AMD_INPUT_ERROR, kNoG2Plan);
  const TapPoints pts = {&g.ws.buckets, &g.ws.partial, sizeof(PtI2), sizeof(Jacobian2), sizeof(Jacobian2), tap_g2_bucket,
                         tap_g2_partial};
  return tap_stage_copy(ctx, g.ws, g.last_plan, g.slot.counters(), pts, which, out, bytes);
}

int msm_amd_test_op_g2(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  if (!ctx || op < 0 || (op >= G2RAW_OPS && op != MSM_AMD_G2_RAW_FQ2_SQRT) || count == 0 || count > (1u << 20) || !a || !b ||
      !out)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad test_op_g2 arguments");
  DeviceCall c;
  c.who = __func__;
  c.g2 = true;
  c.all_host(true);
  c.host_in = 3u;
  c.in[0] = a, c.in[1] = b, c.in_bytes[0] = c.in_bytes[1] = count * kG2RawIn * 4;
  c.out = out, c.out_bytes = count * kG2RawOut * 4;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return device_call(ctx, c, [&](hipStream_t st, const CallIo& io) -> int {
    if (op == MSM_AMD_G2_RAW_FQ2_SQRT)
      launch_sqrt_raw(st, true, (const uint32_t*)io.in[0], (uint32_t*)io.out, (uint32_t)count);
    else
      launch_test_op_g2(st, op, (const uint32_t*)io.in[0], (const uint32_t*)io.in[1], (uint32_t*)io.out, (uint32_t)count);
    return MSM_AMD_OK;
  });
}

}  // extern "C"
