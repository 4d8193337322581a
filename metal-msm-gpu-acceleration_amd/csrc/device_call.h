// ---- the blocking vector calls: the point calls of both groups, the transform, the vectors over Fr ------------------------
// One driver for all of them (device_call): the device set, a bounded drain of the ctx's earlier work, every buffer sized
// on the idle ctx before anything is enqueued, host input through the page-locked staging ring, the caller's kernels on
// the main stream (between events when the call is timed), the 64-byte record of a call that has one behind a bounded
// wait, output and reason bytes behind a bounded stream wait.  The test ops and the reference-shaped prepare and sort
// stage entries (calls_stages.hip) run on it as well.  Each call validates its own arguments, takes
// ctx->mu, describes its buffers in a DeviceCall and passes a callable that enqueues its kernels; one that takes the
// finished record, and the kernels that follow it, are optional.
#pragma once
#include <type_traits>

#include "host_ctx.h"

namespace {

struct DeviceCall {
  std::string who;              // the entry point, in every message
  bool g2 = false;              // the buffers are G2State::calls
  bool host = false;            // out / reasons are host memory: written in the staging and copied back
  unsigned host_in = 0;         // bit k: in[k] is host memory and goes through the staging
  bool in_place = false;        // host: the result is written over the staged in[0] and copied back from there
  bool counters = false;        // the record is PointCounters: reset before the kernels, read back behind them
  float* kernel_ms = nullptr;   // optional: the device time of the kernels
  size_t n = 0;                 // reason bytes
  const void* in[3] = {};
  size_t in_bytes[3] = {};
  DeviceBuf* stage[3] = {};     // the staging of in[k] if not CallState::in[k] (G2State::in_points, CallState::pow)
  void* out = nullptr;
  size_t out_bytes = 0;
  uint8_t* reasons = nullptr;   // optional
  struct {
    DeviceBuf* buf;
    size_t bytes;
  } work[2] = {};               // device-side buffers of the kernels
  size_t values_bytes = 0;      // what launch leaves at CallIo::values comes back in CallState::h_values
  void all_host(bool h) { host = h, host_in = h ? 7u : 0u; }
};

// what the kernels of a call see: device memory throughout
struct CallIo {
  const void* in[3];
  void* out;
  uint8_t* reasons;
  PointCounters* counters;
  const void* record;   // the 64 bytes to read back: `counters` of a call that has them; else null, unless launch sets it
  const void* values;   // DeviceCall::values_bytes to read back behind the kernels; launch sets it
};

// ctx->mu is held.  launch(stream, io) enqueues the kernels and returns a status.  A call with a record gets it back
// behind a bounded wait: then(record, device_ms) takes it on the host, and launch2(stream, io), if there is one,
// enqueues the kernels that needed it.  kernel_ms is the time of the one or two spans of kernels, without the host's
// step between them; an event is recorded only for a call that has counters or asks for the time (one hipEventRecord
// costs ~6 us of stream idle time, see EV_START above).
template <class Launch, class Then, class Launch2>
int device_call(msm_amd_ctx* ctx, const DeviceCall& c, Launch launch, Then then, Launch2 launch2) {
  constexpr bool two_spans = !std::is_null_pointer<Launch2>::value;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return fail(ctx, rc, c.who + ": " + ctx->last_error);
  if (!drain_or_mark_stalled(ctx))
    return fail(ctx, MSM_AMD_PIPELINE_ERROR, c.who + ": device busy past the wait bound of " +
                                                 std::to_string(ctx->wait_timeout_ms) + " ms (msm_amd_synchronize waits again)");
  CallState& s = c.g2 ? ctx->g2.calls : ctx->calls;
  hipStream_t st = ctx->stream;
  int rc;
  // the ctx is idle: the first call creates the record and the events, and every buffer of this call is sized now
  if (!s.ready) {
    if ((rc = ensure(ctx, s.record, sizeof(PointCounters)))) return rc;
    if (!s.h_record) HIP_TRY(ctx, hipHostMalloc((void**)&s.h_record, sizeof(PointCounters), hipHostMallocDefault));
    for (hipEvent_t& e : s.ev)
      if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    s.ready = true;
  }
  for (const auto& w : c.work)
    if (w.buf && (rc = ensure(ctx, *w.buf, w.bytes))) return rc;
  if (c.values_bytes > s.h_values_cap) {
    if (s.h_values) (void)hipHostFree(s.h_values);
    s.h_values = nullptr, s.h_values_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&s.h_values, c.values_bytes, hipHostMallocDefault));
    s.h_values_cap = c.values_bytes;
  }
  DeviceBuf* stage[3];
  for (int k = 0; k < 3; ++k) {
    stage[k] = c.stage[k] ? c.stage[k] : &s.in[k];
    if ((c.host_in >> k & 1) && (rc = ensure(ctx, *stage[k], c.in_bytes[k]))) return rc;
  }
  if (c.host && !c.in_place && (rc = ensure(ctx, s.out, c.out_bytes))) return rc;
  if (c.host && c.reasons && (rc = ensure(ctx, s.reasons, c.n))) return rc;
  CallIo io = {{c.in[0], c.in[1], c.in[2]}, c.out, c.reasons, (PointCounters*)s.record.p, c.counters ? s.record.p : nullptr,
               nullptr};
  for (int k = 0; k < 3; ++k)
    if ((c.host_in >> k & 1) && c.in_bytes[k]) {
      if ((rc = staged_upload(ctx, stage[k]->p, c.in[k], c.in_bytes[k], st))) return rc;
      io.in[k] = stage[k]->p;
    }
  if (c.host && c.out_bytes) io.out = c.in_place ? const_cast<void*>(io.in[0]) : s.out.p;
  if (c.host && c.reasons) io.reasons = (uint8_t*)s.reasons.p;
  const bool timed = c.counters || c.kernel_ms;
  auto span = [&](auto& enqueue, int first_event) -> int {
    if (timed) HIP_TRY(ctx, hipEventRecord(s.ev[first_event], st));
    if (int lrc = enqueue(st, io)) return lrc;
    HIP_TRY(ctx, hipGetLastError());
    if (timed) HIP_TRY(ctx, hipEventRecord(s.ev[first_event + 1], st));
    return MSM_AMD_OK;
  };
  if (c.counters) launch_point_reset(st, io.counters);
  if ((rc = span(launch, 0))) return rc;
  const bool has_record = io.record != nullptr;
  bool pending = true;   // work enqueued and not waited for
  float ms = 0.0f;
  if (has_record) {
    HIP_TRY(ctx, hipMemcpyAsync(s.h_record, io.record, sizeof(PointCounters), hipMemcpyDeviceToHost, st));
    if ((rc = sync_stream_bounded(ctx, st, c.who.c_str()))) return rc;
    if (timed) ms = event_span(s.ev[0], s.ev[1]);
    then(s.h_record, ms);
    if constexpr (two_spans) {
      if ((rc = span(launch2, 2))) return rc;
    } else {
      pending = false;
    }
  }
  if (c.host && c.out_bytes) HIP_TRY(ctx, hipMemcpyAsync(c.out, io.out, c.out_bytes, hipMemcpyDeviceToHost, st));
  if (c.host && c.reasons) HIP_TRY(ctx, hipMemcpyAsync(c.reasons, io.reasons, c.n, hipMemcpyDeviceToHost, st));
  if (c.values_bytes) HIP_TRY(ctx, hipMemcpyAsync(s.h_values, io.values, c.values_bytes, hipMemcpyDeviceToHost, st));
  if ((c.host && (c.out_bytes || c.reasons)) || c.values_bytes) pending = true;
  if (pending && (rc = sync_stream_bounded(ctx, st, c.who.c_str()))) return rc;
  if (timed && !has_record) ms = event_span(s.ev[0], s.ev[1]);
  if (timed && two_spans) ms += event_span(s.ev[2], s.ev[3]);
  if (c.kernel_ms) *c.kernel_ms = ms;
  return MSM_AMD_OK;
}

template <class Launch, class Then>
int device_call(msm_amd_ctx* ctx, const DeviceCall& c, Launch launch, Then then) {
  return device_call(ctx, c, launch, then, nullptr);
}

template <class Launch>
int device_call(msm_amd_ctx* ctx, const DeviceCall& c, Launch launch) {
  return device_call(ctx, c, launch, [](const uint8_t*, float) {}, nullptr);
}

// The point calls: n records (and reason bytes) of host or of device memory throughout; null_arg: some required
// pointer is null.  done(counters, device_ms) takes the result of a call with counters (and the empty counters of a
// call with n == 0, whatever its kind).
template <class Launch, class Done>
int point_call(msm_amd_ctx* ctx, const DeviceCall& c, bool null_arg, Launch launch, Done done) {
  if (c.n > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": n >= 2^32");
  if (c.n == 0) {
    done(point_counters_empty(), 0.0f);
    return MSM_AMD_OK;
  }
  if (null_arg) return fail(ctx, MSM_AMD_INPUT_ERROR, c.who + ": null pointer with n > 0");
  std::lock_guard<std::mutex> lk(ctx->mu);
  return device_call(ctx, c, launch, [&](const uint8_t* record, float ms) {
    PointCounters pc;
    std::memcpy(&pc, record, sizeof pc);
    done(pc, ms);
  });
}

}  // namespace
