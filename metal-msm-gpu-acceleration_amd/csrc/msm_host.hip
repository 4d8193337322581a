// Host driver + C ABI of libmsm_amd.so (see include/msm_amd.h).
//
// Replaces the reference's L2-L4 layers for the MSM path: MetalState (src/metal/abstraction/state.rs),
// MetalMsmConfig/Instance + encode_instances + exec_metal_commands + gpu_msm_h2c_sync
// (src/metal/msm.rs:28-349) and the stage drivers (src/metal/msm/*.rs).  The stages of one MSM are enqueued on
// FOUR HIP streams (front end / accumulate / two alternating reduce streams, ordered by events) with no host
// synchronisation in between (the reference blocks after every stage: prepare_buckets_indices.rs:35-36,
// bucket_wise_accumulation.rs:104-105, sum_reduction.rs:80-81); the only device->host hand-off is the
// (c-2)*W partial window points for the host Horner pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/msm_amd.h"
#include "device_common.hip.h"
#include "launch.h"
#include "launch_g2.h"
#include "launch_check.h"
#include "launch_compress.h"
#include "launch_mul.h"
#include "launch_fr.h"
#include "launch_ntt.h"
#include "launch_nttp.h"
#include "host_fq64.h"
#include "test_ops.hip.h"
#include "test_ops_g2.hip.h"

using namespace msm_amd;

namespace {

constexpr uint32_t kModulusBits = 254;   // limbs_conversion.rs:172, :344
constexpr uint32_t kMinWindow = 3, kMaxWindow = 17;   // u16 digits up to 15, u32 digits for 16 and 17
constexpr uint32_t kDefaultBallot = 1;                // sort ranking (Plan::ballot), chosen by profiles/r02_sort_ranking_ab.txt
constexpr size_t kCpuDispatchBelow = 17;              // msm_best: see cpu_dispatch_below()

struct DeviceBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// One hipEventRecord costs ~6 us of stream idle time on this stack (profiles/r02_lone_call_2p18_timeline.txt: 5.7 us
// between two kernels with one event between them, none without), so the accumulate kernel is bracketed by ONE pair
// of events that serves as stage span, kernel span (the roofline figure of bench.py) and start of the reduce span.
enum {
  EV_START = 0, EV_CONVERT, EV_DIGITS, EV_SORT, EV_ACC_S, EV_ACC, EV_REDUCE, EV_COUNT,
  EV_ACC_K0 = EV_ACC_S, EV_ACC_K1 = EV_ACC, EV_RED_S = EV_ACC
};

// The host side of one instance, G1 or G2: its stage events and the page-locked landing place of its results --
// h_partial_cap partial points of ext_bytes each (Jacobian or Jacobian2), then one more record of that size that
// receives the plan counters of the instance (work-item statistics for timings and the stage tap).
struct InstanceSlot {
  hipEvent_t ev[EV_COUNT];
  uint8_t* h_partial = nullptr;   // pinned
  size_t h_partial_cap = 0, ext_bytes = 0;
  bool has_events = false;
  PlanCounters counters() const {
    PlanCounters pc;
    std::memcpy(&pc, h_partial + h_partial_cap * ext_bytes, sizeof pc);
    return pc;
  }
};

}  // namespace

// Device buffers of one in-flight MSM.  A ctx owns kWorkspaces (4) of them and uses them round-robin: the window
// reduction of instance i runs on a side stream while the main stream accumulates instance i+1 and the front
// stream already sorts instance i+2, each in its own workspace.  The reduction is latency-bound (about 25 dependent point additions on a few hundred
// workgroups) and so is the sort front-end; running them side by side hides the shorter of the two.  (Running
// whole instances on parallel streams was tried and gained little: a resident accumulate grid keeps the
// 1024-thread sort workgroups of the other stream from being placed at all.)
struct Workspace {
  DeviceBuf digits, coarse_cnt, region_start, tmp_idx, tmp_fine, tmp_idx2, tmp_fine2, mid_cnt, region_start2, bsize, bstart, istart, win_items, size_bins, sorted,
      order, multi_list, redo_list, counters, bases29, buckets, item_partials, S, T, partial, conv_scalars, conv_points,
      conv_tmp;
  // hand-off events between the streams of the ctx (null in a workspace that one stream alone uses: G2State::ws)
  hipEvent_t front_done = nullptr;    // front stream: sorted indices / work items of this workspace are ready
  hipEvent_t acc_done = nullptr;      // main stream: buckets of this workspace are complete (incl. combine)
  hipEvent_t reduce_done = nullptr;   // reduce stream: buckets / partial of this workspace are free again
  bool acc_pending = false, reduce_pending = false;
};

// One set of bases a host-slice caller keeps handing over (msm_amd_set_bases_cache): the converted device copy, keyed
// by (host pointer, n, layout) and guarded by sampled checksums of the host records.  The records are cut into
// S = n / 1024 interleaved phases (record i belongs to phase i mod S); every phase is hashed when the entry is filled,
// and every later call re-hashes phase 0 and one rotating phase of the caller's memory (~2 k records, tens of
// microseconds): a changed array at an unchanged address is caught at once if it touches phase 0 and within S calls
// otherwise.  The caller's contract stays "same pointer, same bases"; the checksums are the safety net.
struct BasesCacheEntry {
  const void* host = nullptr;
  size_t n = 0;
  int layout = 0;
  std::vector<uint64_t> phase_hash;
  std::vector<uint64_t> chunk_hash;   // kCacheChunks contiguous slices: the FULL verification (bases_cache_verify)
  void* d_prepared = nullptr;   // n x AffPacked
  uint64_t last_use = 0;        // bases_cache_call of the last call that used it
  uint64_t wanted_by = 0;       // bases_cache_call of the last call whose arguments name it (bases_cache_reserve)
  uint32_t next_phase = 1;
};

// Upload of PAGEABLE host memory through the library's own page-locked ring: helper threads copy 4 MiB chunks into
// pinned slots, each chunk goes on by DMA as soon as it is there.  The runtime's staged copy of pageable memory blocks
// the calling thread either way; on the HIP 7.0 runtime (the one inside the PyTorch wheel) it also serialises with
// the kernels of the other streams, this path does not (a page-locked source never did).
struct Stager {
  static constexpr size_t kChunk = (size_t)4 << 20;
  static constexpr int kSlots = 4, kMaxHelpers = 7;
  int n_helpers = 3;   // MSM_AMD_STAGE_HELPERS = 1 .. 7 overrides (measured: profiles/r03_staged_upload_helpers.txt)
  void* slot[kSlots] = {};
  hipEvent_t sent[kSlots] = {};
  bool busy[kSlots] = {};
  int next = 0;
  bool ready = false;
  // helper threads: copy parts 1 .. n_helpers of the current chunk (the caller copies part 0)
  std::vector<std::thread> helpers;
  std::mutex m;
  std::condition_variable wake, finished;
  const uint8_t* src = nullptr;
  uint8_t* dst = nullptr;
  size_t bytes = 0;
  std::atomic<uint64_t> generation{0};
  int pending = 0;
  bool quit = false;
};

// The uploads of a host-slice batch run on a helper thread, one instance ahead of the thread that submits kernels: a
// copy from pageable memory blocks whoever issues it (the runtime stages it, or staged_upload does), and on the
// submitting thread that was 1.3 ms per 2^20-point instance during which nothing else got enqueued.
struct UploadJob {
  void* d_scalars = nullptr;
  const void* h_scalars = nullptr;
  size_t scalar_bytes = 0;
  void* d_points = nullptr;
  const void* h_points = nullptr;
  size_t point_bytes = 0;          // 0: the points are resident (prepared bases, tables, a bases-cache hit)
  hipEvent_t wait_for = nullptr;   // GPU-side: the previous reader of the staging set (nullptr: none)
  hipEvent_t done = nullptr;       // recorded on the copy stream behind the copies
};
struct Uploader {
  std::thread th;
  std::mutex m;
  std::condition_variable cv, cv_idle;
  UploadJob job;
  bool has_job = false, busy = false, quit = false, started = false;
  int status = 0;
  std::string error;
};

constexpr int kWorkspaces = 4;
constexpr int kReduceStreams = 2;
constexpr int kMaxBatches = 4;   // batches that may be in flight between submit and wait

struct Batch {
  std::vector<InstanceSlot> slots;
  std::vector<Plan> plans;
  std::vector<int> ws_index;   // workspace each instance ran in (read by the msm_amd_test_* stage tap only)
  std::vector<size_t> first_index;   // bounded calls: index of each instance's first record in the caller's vector (a
                                     // call cut into point ranges, run_split), for the message of a violated bound
  bool lone = false;
  void* out = nullptr;
  size_t n_inst = 0;
  bool active = false;
  bool abandoned = false;   // a blocking entry point gave up waiting for it (wait timeout): released once the device is idle
};

// What the handle kinds share: one device allocation.  Handles are validated by membership in the live list of
// their kind (find_handle), never by dereferencing the caller's pointer; each kind is a type and a live list of its own,
// so that a G1 table handle is no G2 table handle, neither is a transform domain, and the reverse.
struct DeviceHandle {
  void* d_mem = nullptr;
  size_t bytes = 0;
};

// Precomputed window tables of one set of bases (msm_amd_tables_*, msm_amd_g2_tables_*): d_mem[w * n + i] = 2^(c w) P_i,
// W * n AffPacked (G1, msm_amd_ctx::live_tables) or Aff2Packed (G2, msm_amd_ctx::live_g2_tables).
struct TablesRecord : DeviceHandle {
  size_t n = 0;
  uint32_t c = 0, W = 0;
};
struct msm_amd_tables : TablesRecord {};
struct msm_amd_g2_tables : TablesRecord {};

// The twiddles of one (root, log_n) (msm_amd_ntt_domain_*, msm_amd_ctx::live_ntt): d_mem[j] = omega^j, j < n/2, Montgomery.
struct msm_amd_ntt_domain : DeviceHandle {
  int root = 0;
  uint32_t log_n = 0;
  u256 omega{};
};

// A sparse matrix over Fr (msm_amd_fr_matrix_*, msm_amd_ctx::live_fr_mat): d_mem is the image of fr_mat_image, planned at
// the ctx's (fr_mat_long, fr_mat_seg_log) of the build.
struct msm_amd_fr_matrix : DeviceHandle {
  uint64_t n_rows = 0, n_cols = 0, nnz = 0, n_distinct = 0;
  uint32_t long_rows = 0;
  FrMatPlan plan{};
  FrMatImage at{};
};

// The constants of one Poseidon instance (msm_amd_poseidon_params_*, msm_amd_ctx::live_poseidon): d_mem is the constants image
// of fr_poseidon.hip.h, reduced Montgomery residues.
struct msm_amd_poseidon_params : DeviceHandle {
  uint32_t t = 0, r_f = 0, r_p = 0;
};

// Buffers of the blocking vector calls (device_call below): the staging of the host-buffer forms, the 64-byte record a
// call reads back with its page-locked copy (the PointCounters of a check, decompress or compress call; T and the zero
// count of a batch inversion), the device-side work buffers and two pairs of events behind kernel_ms.  Every such call
// starts on an idle ctx and blocks until it is done, so one set serves the G1 point calls, the transform and the Fr
// vector calls; G2State has a second one, so that a G2 call touches G2State only.
struct CallState {
  DeviceBuf in[3], out, reasons;   // staging of host inputs, output and reason bytes
  DeviceBuf record;                // PointCounters
  DeviceBuf table, xyzz;           // mul_points: the fixed-base table, the XYZZ records of one chunk of outputs
  DeviceBuf scratch, pow;          // transform: the ONE batch-sized scratch of a plan with more than one pass, the powers of a shift;
                                   // transform over points: `scratch` holds the two packed work arrays, back to back (2 x 64 n bytes)
  DeviceBuf work;                  // Fr scan and inversion: the tile totals (fr_scan_plan, fr_inv_plan); the partial sums of
                                   // the split rows of a sparse product (fr_mat_plan); the partial sums of a sumcheck round,
                                   // the levels of a multilinear evaluation, the turns of a LOW bind (fr_mle.hip.h)
  uint8_t* h_record = nullptr;     // pinned, 64 bytes
  uint8_t* h_values = nullptr;     // pinned: the values a call reads back beside its output (p_v(z) of the polynomial calls)
  size_t h_values_cap = 0;
  hipEvent_t ev[4] = {};           // start and end of the first and of the second span
  bool ready = false;              // record, h_record and ev exist
  // everything but the record: what a kernel reads only after its own call has written it, so what
  // msm_amd_test_fill_workspaces may poison
  std::array<DeviceBuf*, 10> scratch_bufs() { return {&in[0], &in[1], &in[2], &out, &reasons, &table, &xyzz, &scratch, &pow, &work}; }
  // msm_amd_destroy, with its own ways of releasing a buffer and an event
  template <class KillBuf, class KillEvent>
  void release(KillBuf kill_buf, KillEvent kill_event) {
    kill_buf(record);
    for (DeviceBuf* b : scratch_bufs()) kill_buf(*b);
    for (hipEvent_t& e : ev) kill_event(e);
    if (h_record) (void)hipHostFree(h_record);
    if (h_values) (void)hipHostFree(h_values);
    h_record = h_values = nullptr;
    h_values_cap = 0;
    ready = false;
  }
};
static_assert(sizeof(PointCounters) == 64, "CallState::record and h_record hold one PointCounters");

// State of the G2 MSM (msm_amd_msm_g2*): one blocking call at a time on the main stream, through the instance body of
// G1 (enqueue_instance) in a workspace and a slot of its own -- a G2 call never touches what a G1 instance of the same
// ctx may still be using.  `ws` is used on the main stream only and therefore has no hand-off events.
struct G2State {
  Workspace ws;
  InstanceSlot slot;
  DeviceBuf in_scalars, in_points;   // staging of host inputs
  CallState calls;   // the G2 point calls; msm_amd_g2_check_points stages host points in in_points above
  // Stage tap (msm_amd_test_g2_last_plan / msm_amd_test_g2_stage_copy): the plan of the last run_msm_g2, valid only
  // while that call was the last one and succeeded.  Its plan counters are in `slot`, behind the partial points.
  Plan last_plan{};
  bool has_last_plan = false;
};

struct msm_amd_ctx {
  int device = 0;
  hipStream_t stream = nullptr;          // main stream: conversion, digits, sort, accumulate; stage entry points
  hipStream_t reduce_streams[kReduceStreams] = {};   // side streams: window reduction + copy of the partial points.
                                         // Consecutive instances alternate between them: the tail of an instance is a
                                         // chain of latency-bound kernels that is as long as one accumulate, so two
                                         // of them must be able to overlap.  (More streams than the four hardware
                                         // queues HIP gives a process -- main, front, two reduce -- share a queue
                                         // with the accumulate grid and wait behind it: measured, 1.6x slower.)
  bool alt_reduce = true;                // MSM_AMD_ALT_REDUCE=0: one reduce stream
  int acc_variant = 1;                   // accumulate kernel build (launch_accumulate): 1 shipped, 0 without the register pin; experiments build: 2..12
  uint32_t acc_lds = 0;                  // LDS bytes per accumulate workgroup: caps its waves per CU (MSM_AMD_ACC_LDS)
  uint32_t seq = 0;
  hipStream_t front_stream = nullptr;    // side stream: conversion, digits, sort, work-item planning
  hipStream_t copy_stream = nullptr;     // host-buffer entry points: uploads (DMA when the caller registered its buffers)
  hipEvent_t uploaded[2] = {nullptr, nullptr};   // per staging set: the upload on copy_stream has finished
  std::vector<std::pair<const void*, size_t>> host_regs;   // msm_amd_host_register
  bool overlap_reduce = true;            // MSM_AMD_OVERLAP_REDUCE=0 puts the reduction on the main stream
  bool overlap_front = true;             // MSM_AMD_OVERLAP_FRONT=0 puts the front end on the main stream
  bool lone_single_stream = true;        // MSM_AMD_LONE_SINGLE_STREAM=0: a lone instance uses the stream split too
  Workspace ws[kWorkspaces];
  G2State g2;
  CallState calls;   // the G1 point calls, the transform and the Fr vector calls
  size_t mul_chunk = (size_t)1 << 18;   // outputs per chunk of a mul_points call (MSM_AMD_MUL_CHUNK), a multiple of kMulNormGroup
  std::mutex mu;
  std::string last_error;
  uint32_t forced_window = 0;
  // The width of the instances being submitted (msm_amd_msm_bounded* set it for the length of their call, under mu;
  // enqueue_msm / run_msm_g2 plan with it); range_first, if set, holds the first record index of every instance
  // submitted next (run_split), range_at the instance submit_batch_device starts from.
  WidthBound bound{};
  const size_t* range_first = nullptr;
  size_t range_at = 0;
  std::vector<msm_amd_tables*> live_tables;
  std::vector<msm_amd_g2_tables*> live_g2_tables;
  std::vector<msm_amd_ntt_domain*> live_ntt;
  std::vector<msm_amd_fr_matrix*> live_fr_mat;
  std::vector<msm_amd_poseidon_params*> live_poseidon;
  uint32_t fr_tile_log = kFrTileLog;     // records per tile of a scan, as a power of two (MSM_AMD_FR_TILE_LOG)
  uint32_t fr_mat_long = kFrMatLong;     // rows of a sparse matrix above this many entries take the wave path (MSM_AMD_FR_MAT_LONG)
  bool fr_mat_signs = false;             // the product kernels that skip the product for values 1 and r - 1 (MSM_AMD_FR_MAT_SIGNS)
  uint32_t fr_mat_seg_log = kFrMatSegLog;   // entries per wave of that path, as a power of two (MSM_AMD_FR_MAT_SEG_LOG)
  uint32_t fr_mle_chunk_log = kFrMleChunkLog;   // pairs per wave of a sumcheck round, as a power of two (MSM_AMD_FR_MLE_CHUNK_LOG)
  uint32_t poseidon_top_log = kPoseidonTopLog;   // tree levels of at most 2^this nodes share the last workgroup (MSM_AMD_POSEIDON_TOP_LOG)
  uint32_t ntt_tile_log = kNttTileLog;   // elements per workgroup of a transform pass, as a power of two (MSM_AMD_NTT_TILE_LOG)
  int next_ws = 0;
  DeviceBuf scratch_a, scratch_b, scratch_c, scratch_b2, scratch_c2;
  Batch batches[kMaxBatches];
  int last_waited = -1;   // batch of the last successful wait_batch (msm_amd_test_last_plan / msm_amd_test_stage_copy)
  msm_amd_timings timings{};
  float after_sort_state = -1.0f;   // timings.reserved2[1] of the next wait (see msm_amd_gpu_msm_h2c_sync)
  float after_sort_lead_ms = 0.0f;  // timings.reserved2[2]: device time from the callback to the end of accumulation
  hipEvent_t after_sort_mark = nullptr;   // recorded on the idle copy stream the moment the callback is about to run
  // Scalars staged by a single-instance entry point (msm_prepared, msm_tables, gpu_msm_h2c_sync): the upload is on
  // `upload_stream`; whichever stream enqueue_msm then picks for the front end waits for `upload_done` unless it IS
  // that stream (the entry point cannot know: run_batch_device may turn the call into pipelined point ranges).
  hipEvent_t upload_done = nullptr;
  hipStream_t upload_stream = nullptr;
  bool upload_pending = false;
  // Upper bound of every host wait for a GPU event (MSM_AMD_WAIT_TIMEOUT_MS, msm_amd_set_wait_timeout_ms; 0 = none).
  // A wait that runs into it returns MSM_AMD_PIPELINE_ERROR naming the event and instance not reached; the batch
  // stays in flight (`stalled`), and the next entry point first checks whether the device has caught up.
  uint32_t wait_timeout_ms = 60000;
  bool stalled = false;
  // Opt-in cache of converted bases for the host-slice entry points (msm_amd_set_bases_cache, MSM_AMD_BASES_CACHE_MB)
  std::vector<BasesCacheEntry> bases_cache;
  size_t bases_cache_budget = 0, bases_cache_bytes = 0;
  // 0 = sampled verification of a hit (phase 0 + one rotating phase of the caller's records), 1 = every record
  // re-hashed on every hit (msm_amd_set_bases_cache_verify, MSM_AMD_BASES_CACHE_VERIFY=full)
  int bases_cache_verify = 0;
  uint64_t bases_cache_call = 0, bases_cache_hits = 0, bases_cache_misses = 0, bases_cache_invalidations = 0;
  // device room for cache entries, allocated at the START of a host-slice call while the ctx is idle (nothing is ever
  // allocated under work in flight) and taken by bases_cache_insert when the instance is dispatched
  struct CacheReserve {
    const void* host;
    size_t n;
    int layout;
    void* d;
  };
  std::vector<CacheReserve> cache_reserve;
  AffPacked* convert_into = nullptr;   // enqueue_msm writes the converted bases of the next instance here (a cache fill)
  bool staging_points = false;         // the next instance's points sit in a staging set that is uploaded into again once
                                       // its digits are done (run_batch_host): accumulate cannot gather them in place
  // Device buffers replaced by bigger ones while work was in flight.  hipFree synchronises the whole device: inside
  // a submit it would stall the pipeline and, on a device that does not answer, block without bound.  They are
  // freed when the ctx has nothing in flight (reap_graveyard) or at msm_amd_destroy.
  std::vector<void*> graveyard;
  Stager stager;
  Uploader uploader;
  int staged_uploads = -1;   // -1 = decide by the runtime version (stage_pageable()), 0 / 1 = MSM_AMD_STAGED_UPLOAD
};

namespace {

std::mutex g_global_mu;
msm_amd_ctx* g_global_ctx = nullptr;

// A helper thread of the library (the uploader) reports through its own string: ctx->last_error belongs to the thread
// that holds ctx->mu.
thread_local std::string* tl_error_sink = nullptr;

int fail(msm_amd_ctx* ctx, int status, const std::string& msg) {
  if (tl_error_sink) *tl_error_sink = msg;
  else if (ctx) ctx->last_error = msg;
  return status;
}

// Wait for everything this ctx has enqueued (error paths and set-up steps that reuse workspace 0).
void drain_streams(msm_amd_ctx* ctx) {
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  (void)hipStreamSynchronize(ctx->front_stream);
  (void)hipStreamSynchronize(ctx->stream);
  for (hipStream_t rs : ctx->reduce_streams) (void)hipStreamSynchronize(rs);
  (void)hipGetLastError();
}

// All streams of the ctx idle?  (hipStreamQuery never blocks)
bool streams_idle(msm_amd_ctx* ctx) {
  hipStream_t all[] = {ctx->copy_stream, ctx->front_stream, ctx->stream, ctx->reduce_streams[0], ctx->reduce_streams[1]};
  bool idle = true;
  for (hipStream_t s : all)
    if (s && hipStreamQuery(s) != hipSuccess) idle = false;
  (void)hipGetLastError();
  return idle;
}

// drain_streams with the ctx's wait bound: false if the device did not get there in time.
bool drain_streams_bounded(msm_amd_ctx* ctx) {
  if (ctx->wait_timeout_ms == 0) {
    drain_streams(ctx);
    return true;
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (!streams_idle(ctx)) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ctx->wait_timeout_ms)) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  return true;
}

// Error paths and set-up steps: the bounded drain; a device that does not get there leaves the ctx marked stalled (the
// next entry point checks whether it has caught up) instead of holding the caller.
bool drain_or_mark_stalled(msm_amd_ctx* ctx);
int sync_stream_bounded(msm_amd_ctx* ctx, hipStream_t st, const char* what);

// hipEventSynchronize may park the thread (it did, for more than a millisecond, inside a process that also hosts
// torch's thread pools) and it waits without bound: a device that stalls would block the caller of a blocking MSM
// for ever, where the reference's call always returns (msm.rs:237-349).  The waits on the critical path therefore
// poll the event -- spinning for the first few milliseconds, then with short sleeps -- up to `timeout_ms`
// (0 = unbounded) and report hipErrorNotReady when the bound is reached.
hipError_t wait_event(hipEvent_t ev, uint32_t timeout_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return hipSuccess;
    if (q != hipErrorNotReady) {
      (void)hipGetLastError();
      return q;
    }
    (void)hipGetLastError();
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (timeout_ms && waited > std::chrono::milliseconds(timeout_ms)) return hipErrorNotReady;
    if (waited > std::chrono::milliseconds(4))
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    else
      __builtin_ia32_pause();
  }
}

uint32_t default_wait_timeout_ms() {
  if (const char* e = std::getenv("MSM_AMD_WAIT_TIMEOUT_MS")) return (uint32_t)std::strtoul(e, nullptr, 10);
  return 60000;
}

const char* const kEventNames[] = {"start", "convert", "digits", "sort", "accumulate-start", "accumulate", "reduce"};

#define HIP_TRY(ctx, expr)                                                                        \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      (void)hipGetLastError();                                                                    \
      return fail(ctx, MSM_AMD_PIPELINE_ERROR,                                                    \
                  std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +         \
                      std::to_string(__LINE__) + ")");                                            \
    }                                                                                             \
  } while (0)

// A wait on this ctx ran into its bound earlier.  Before anything new is enqueued: has the device caught up?  If every
// stream is idle the batches a blocking entry point abandoned are released; otherwise the call fails like the wait did.
int recover_if_stalled(msm_amd_ctx* ctx) {
  if (!ctx->stalled) return MSM_AMD_OK;
  if (!streams_idle(ctx))
    return fail(ctx, MSM_AMD_PIPELINE_ERROR,
                "the device is still busy with work whose wait timed out earlier (msm_amd_synchronize waits again; "
                "msm_amd_destroy gives the ctx up)");
  for (Batch& b : ctx->batches)
    if (b.abandoned) b.active = b.abandoned = false;
  ctx->stalled = false;
  return MSM_AMD_OK;
}

// Nothing of this ctx is in flight (every submitted batch has been waited for): outgrown buffers can go.
void reap_graveyard(msm_amd_ctx* ctx) {
  if (ctx->graveyard.empty() || ctx->stalled) return;
  for (const Batch& b : ctx->batches)
    if (b.active) return;
  for (void* p : ctx->graveyard) (void)hipFree(p);
  (void)hipGetLastError();
  ctx->graveyard.clear();
}

// hipMalloc / hipHostMalloc / hipFree / hipHostFree may wait for the device (hipFree always does).  With work in flight
// on a device that does not answer they would block without bound, before any bounded wait is reached -- so nothing
// is allocated or released while the ctx has work in flight: a buffer that must grow first waits, WITH the ctx's wait
// bound, for the ctx's streams to run empty, and the call fails with MSM_AMD_PIPELINE_ERROR if they do not.  (On a
// healthy device this costs a pipeline drain on the first use of a workspace, never in steady state.)
int quiesce_for_allocation(msm_amd_ctx* ctx, const char* what) {
  if (streams_idle(ctx)) return MSM_AMD_OK;
  if (drain_streams_bounded(ctx)) return MSM_AMD_OK;
  ctx->stalled = true;
  return fail(ctx, MSM_AMD_PIPELINE_ERROR,
              std::string("device busy past the wait bound of ") + std::to_string(ctx->wait_timeout_ms) +
                  " ms: cannot grow " + what + " while earlier work is in flight (msm_amd_synchronize waits again)");
}

// hipStreamSynchronize with the ctx's wait bound (the stream is polled): PIPELINE_ERROR, ctx marked stalled, when the
// device does not get there.
int sync_stream_bounded(msm_amd_ctx* ctx, hipStream_t st, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess) return MSM_AMD_OK;
    (void)hipGetLastError();
    if (q != hipErrorNotReady)
      return fail(ctx, MSM_AMD_PIPELINE_ERROR, std::string("hipStreamQuery (") + what + "): " + hipGetErrorString(q));
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (ctx->wait_timeout_ms && waited > std::chrono::milliseconds(ctx->wait_timeout_ms)) {
      ctx->stalled = true;
      return fail(ctx, MSM_AMD_PIPELINE_ERROR, "timed out after " + std::to_string(ctx->wait_timeout_ms) +
                                                   " ms waiting for the stream (" + what + ")");
    }
    if (waited > std::chrono::milliseconds(2)) std::this_thread::sleep_for(std::chrono::microseconds(50));
    else __builtin_ia32_pause();
  }
}

bool drain_or_mark_stalled(msm_amd_ctx* ctx) {
  if (drain_streams_bounded(ctx)) return true;
  ctx->stalled = true;
  return false;
}

int ensure(msm_amd_ctx* ctx, DeviceBuf& b, size_t bytes) {
  if (bytes <= b.cap) return MSM_AMD_OK;
  if (int rc = quiesce_for_allocation(ctx, "a device workspace")) return rc;
  if (b.p) ctx->graveyard.push_back(b.p);   // freed later, see msm_amd_ctx::graveyard
  b.p = nullptr;
  b.cap = 0;
  // grow by 25% to avoid re-allocating for every slightly larger instance
  const size_t want = bytes + bytes / 4;
  HIP_TRY(ctx, hipMalloc(&b.p, want));
  b.cap = want;
  return MSM_AMD_OK;
}

uint32_t floor_log2(size_t n) {
  uint32_t l = 0;
  while ((n >> (l + 1)) != 0) ++l;
  return l;
}

uint32_t auto_window(size_t n) {
  // The reference uses 3 below 32 points and 15 from there on (msm.rs:137-141).  Measured on MI355X in pipelined
  // batches (ms per MSM, round 2 -- the row / column-sum reduction made buckets cheaper, which moved every
  // boundary one size down): 2^12 c=5 0.23 | 2^14 c=5 0.24 | 2^16 c=13 0.33 | 2^18 c=15 0.47 (16: 0.50) |
  // 2^19 c=16 0.79 (15: 0.80, 17: 0.84) | 2^20 c=17 1.41 (16: 1.43, 15: 1.54) | 2^21 c=17 2.72 (16: 2.83) |
  // 2^22 c=17 5.82 (16: 6.21).  Windows whose TOP digit is narrow are traps: the n entries of the top window then
  // share a handful of buckets (c = 14 leaves 2 bits for the top window of a 254-bit scalar, c = 11 one bit: 2^17
  // points cost 1.2 ms with c = 10 or 11, 0.38 with 15).
  if (n < 32) return 3;   // msm.rs:137-138
  const uint32_t l = floor_log2(n);
  if (l <= 14) return 5;
  if (l <= 18) return 15;   // 2^16 in batches of 40 after the 64-bit host pass: c=15 0.207, c=13 0.233, c=16 0.246 ms per MSM
  if (l == 19) return 16;   // u32 digits from here on
  return kMaxWindow;
}

// Window size of a LONE call (one instance, nothing else in flight: lone_call()).  The pipelined policy above minimises
// GPU work per MSM; a lone call is a chain of launches and of dependent point additions, where a wide window costs
// little (the window reduction is a fixed number of levels, the accumulate kernel is far from filling the machine)
// and a narrow top window costs a lot (split buckets -> the combine pass).  Median ms of one blocking device-resident
// call on MI355X (tools/lone_latency.py, profiles/r02_lone_call_window_sweep.txt), best | pipelined policy:
//   2^8 c=8 0.346 | c=5 0.357     2^12 c=8 0.446 | c=5 0.538     2^14 c=15 0.487 | c=5 0.596
//   2^16 c=15 0.543 | c=13 0.661  2^18 c=15 0.810 (16: 0.796)    2^19 c=17 1.201 | c=16 1.253
uint32_t auto_window_lone(size_t n) {
  if (n < 32) return 3;
  const uint32_t l = floor_log2(n);
  if (l <= 6) return 5;
  if (l <= 12) return 8;
  if (l <= 18) return 15;
  return kMaxWindow;
}

// Window of a bounded call (msm_amd_msm_bounded*).  254 bits: the two policies above.  Below: read from the sweep of every
// window 3..17 at 2^16, 2^18, 2^20, 2^22 points x 1, 8, 16, 32, 64, 128 bits, lone and pipelined, uniform scalars below
// 2^bits on prepared bases (tools/bounded_bench.py --sweep, profiles/bounded_sweep.txt; ms per MSM).  What it shows:
//  - the window count W = bits / c + 1 decides first: every window sorts and accumulates all n entries.  One window
//    that holds the whole scalar (c = bits + 1, no digit is ever negative) is the fastest form of every width up to 16:
//    8 bits c = 9 (2^22 pipelined 0.57; c = 17: 5.87, c = 5: 2.68), 16 bits c = 17 (2^22: 0.56; c = 9: 0.83, c = 15: 7.4);
//  - the trap of auto_window is much deeper here, because a short scalar has few other windows to hide it behind: a top
//    digit of t = bits - (W - 1) c bits puts n entries into 2^t buckets.  32 bits at 2^20 pipelined: c = 17 (t = 15)
//    0.35, c = 16 (the top window holds the carry alone) 2.2, c = 13 (t = 6) 1.45.  The rule below takes the fewest
//    windows among the c whose top digit is full (t = c - 1) or wide enough that a bucket stays below the longest work
//    item (2^t >= n / 512), and the widest top digit if there is none;
//  - at 2^16 and 2^18 points the 2^16 buckets per window of c = 17 cost more than a fifth window saves: 64 and 128 bits
//    want c = 13 there (2^18 lone 64 bits: 0.455 | c = 17 0.499; 128 bits: 0.674 | 0.791; pipelined 0.233 | 0.282 and
//    0.367 | 0.593), and so does every width in a pipeline of 2^16-point instances (32 bits: c = 11 0.163 | c = 17 0.204);
//  - 128 bits from 2^20 points: c = 10 (W = 13, t = 8) beats the rule's c = 13 at 2^20 (pipelined 1.22 | 1.83, lone
//    1.94 | 2.78) and ties with it at 2^22 (4.31 | 4.15, lone 5.50 | 5.77): no reading of the other cells explains it,
//    so it stands as an exception for the width of a 128-bit challenge alone;
//  - one bit: no window differs by more than the spread (every point lands in slot 1; 2^20 lone 4.49 .. 4.52).
// Cells where the rule is not the fastest window: 2^16 pipelined 16 bits (c = 9 0.179 | c = 6 0.152), 2^18 pipelined
// 16 bits (c = 17 0.199 | c = 9 0.181), 2^22 pipelined 128 bits (above); all others within 3 %.  Sizes below 2^15 were
// not swept: they keep the window of the unbounded call (and still run bits / c + 1 windows of it).
uint32_t auto_window_bounded(size_t n, uint32_t bits, bool lone) {
  const uint32_t c0 = lone ? auto_window_lone(n) : auto_window(n);
  if (bits >= kModulusBits) return c0;
  const uint32_t l = floor_log2(n);
  if (l < 15) return c0;
  uint32_t cmax = (uint32_t)kMaxWindow;
  if ((!lone && l <= 17) || (l <= 18 && bits / kMaxWindow + 1 >= 4)) cmax = 13;
  if (l >= 19 && bits > 124 && bits <= 128) return 10;
  if (bits + 1 <= cmax) return std::max<uint32_t>(kMinWindow, bits + 1);   // one window, every digit positive
  uint32_t best = cmax, best_W = 0, best_t = 0;
  bool best_ok = false;
  for (uint32_t c = 9; c <= cmax; ++c) {
    const uint32_t W = bits / c + 1, t = bits - (W - 1) * c;
    const bool ok = t >= std::min(c - 1, l > 9 ? l - 9 : 0u);
    bool take;
    if (ok != best_ok) take = ok;
    else if (ok) take = best_W == 0 || W < best_W || (W == best_W && l >= 19);   // ties: the larger window from 2^19 points
    else take = best_W == 0 || t > best_t || (t == best_t && l >= 19);
    if (take) best = c, best_W = W, best_t = t, best_ok = ok;
  }
  return best;
}

// `windows` = 0: the per-call pipeline (every signed-digit window owns a bucket set).  `windows` > 0: the
// precomputed-table pipeline of a table with that many windows, where the [W_digits][n_scalars] digit matrix is sorted
// as ONE window of W_digits * n_scalars entries whose "point index" addresses the table entry 2^(c w) P_i directly (the
// table is window-major: a bounded call's W_digits windows are a prefix of it).
// `width`: magnitudes stay below 2^width.width() (scalar_width.hip.h) -- W_digits = width / c + 1 windows, of which the
// top one holds at most c - 1 bits and so absorbs the last carry (254 bits: ceil(255 / c)).  Everything below follows
// from W_digits, W and n.
Plan make_plan(size_t n_scalars, uint32_t c, uint32_t windows = 0, WidthBound width = WidthBound{}) {
  Plan p{};
  p.c = c;
  p.W_digits = width.width() / c + 1;
  if (!(width.bits == kScalarBits && !width.sign)) p.bits = width.bits, p.sign = width.sign;   // 254 unsigned: the unbounded plan
  if (windows) windows = std::min(windows, p.W_digits);
  const size_t n = windows ? n_scalars * windows : n_scalars;
  p.n = (uint32_t)n;
  p.W = windows ? 1u : p.W_digits;
  p.n_scalars = (uint32_t)n_scalars;
  p.wide_digits = c > 15;
  p.lb = std::max(c - 1, (uint32_t)kSegLog);
  p.nb = 1u << p.lb;                  // slot i <-> digit magnitude i + 1 (c = 3 is padded to 8 slots)
  // sort / planning workgroup size: big workgroups are the fastest alone, but they can hardly be placed while
  // an accumulate grid of another instance is resident (they need 16 free wave slots on one CU at once)
  p.front_threads = 1024;
  if (const char* e = std::getenv("MSM_AMD_FRONT_THREADS")) {
    const int v = std::atoi(e);
    if (v == 256 || v == 512 || v == 1024) p.front_threads = (uint32_t)v;
  }
  // sort pass 1: one workgroup per (chunk, window); about 2 x 1024 threads per CU in total
  uint32_t Q = std::max(1u, (512u * (1024u / p.front_threads)) / p.W);
  const uint32_t max_q = (uint32_t)((n + 4095) / 4096);
  Q = std::max(1u, std::min(Q, max_q));
  p.Q = Q;
  p.chunk = (uint32_t)((((n + Q - 1) / Q) + 63) & ~(size_t)63);
  // Sort geometry.  Pass 2 sorts a region inside LDS, so the coarse passes must cut a window into regions of
  // ~16 k entries: T = ceil(log2(n / 16384)) coarse bits.  Up to 7 bits (128 regions) one coarse pass does it
  // (every per-call plan up to 2^21 points); beyond that the bits are split over TWO coarse passes of <= 6 bits
  // each (hb + mb, three-level sort): one pass with 1024 regions keeps too many partially written lines open
  // (2^24 points: 10.2 ms), and 128 regions of 131 k entries force pass 2 to scatter in global memory (6.0 ms).
  uint32_t T = 0;
  while (T + 2 < p.lb && (n >> T) > 16384) ++T;
  uint32_t hb = T, mb = 0;
  if (T > 7) {
    hb = (T + 1) / 2;
    mb = T - hb;
  }
  if (const char* e = std::getenv("MSM_AMD_HB")) {   // experiments: coarse bits of the two-pass sort
    const int v = std::atoi(e);
    if (v >= 0 && (uint32_t)v + 2 <= p.lb) {
      hb = (uint32_t)v;
      mb = 0;
    }
  }
  if (const char* e = std::getenv("MSM_AMD_MB")) {   // experiments: middle-pass bits
    const int v = std::atoi(e);
    if (v >= 0 && hb + (uint32_t)v + 2 <= p.lb) mb = (uint32_t)v;
  }
  p.hb = hb;
  p.mb = mb;
  p.fb = p.lb - hb - mb;
  if (p.fb > 10) {   // the fine histogram is scanned with one bin per thread (<= 1024 bins)
    const uint32_t extra = p.fb - 10;
    p.fb = 10;
    if (p.mb || p.hb + extra > 7) p.mb += extra; else p.hb += extra;
  }
  // what pass 1 leaves in the u16 tmp_fine is mb + fb bits
  while (p.mb + p.fb > 16) {
    ++p.hb;
    --p.mb;
  }
  // Tile-staged scatter (k_sort.hip tile_scatter): 26 % less sort time for ONE huge instance (2^24 points: 7.0 ->
  // 5.2 ms with 1024-thread workgroups), but its 60 VGPRs x 1024 threads cannot be placed beside a resident
  // accumulate grid, so inside a pipeline of instances it loses (headline 695 -> 643 MSM/s; with 512 threads: no
  // difference to the direct scatter).  Used where the sort is not hidden behind another instance's accumulation:
  // per-call plans that need the three-level sort (2^22 points and more).
  p.tiled = (p.mb != 0 && windows == 0) ? 1u : 0u;
  if (const char* e = std::getenv("MSM_AMD_TILED")) p.tiled = std::atoi(e) != 0;
  p.tile_threads = 1024;
  if (const char* e = std::getenv("MSM_AMD_TILE_THREADS")) {
    const int v = std::atoi(e);
    if (v == 256 || v == 512 || v == 1024) p.tile_threads = (uint32_t)v;
  }
  p.ballot = kDefaultBallot;
  if (const char* e = std::getenv("MSM_AMD_BALLOT")) p.ballot = (uint32_t)std::atoi(e) & 3u;
  // front-end traffic: digits_hist_kernel counts the digits it has just made, and where index, sign and fine digit
  // fit one u32 (headline: 20 + 1 + 10 bits) pass 1 hands pass 2 one array instead of two (k_sort.hip)
  p.fused_front = windows == 0;
  p.packed = p.mb == 0 && n >= 1 && floor_log2(std::max<size_t>(n - 1, 1)) + 1 + 1 + p.fb <= 32;
  p.Q2 = 1;
  if (p.mb) {
    const uint32_t regions = p.W << p.hb;
    p.Q2 = std::max(1u, 1024u / regions);
    while (p.Q2 > 1 && (n >> p.hb) / p.Q2 < 4096) p.Q2 >>= 1;
  }
  // accumulate work items: at most CH points each; buckets longer than CH are cut into several items whose partial
  // sums the combine kernels add up (one extra full addition per cut, and a second affine+affine start).  Uniform
  // scalars must split (almost) nothing: CH >= mean + 5 sigma of the Poisson bucket size (2^20 points, c = 16: mean
  // 32, CH = 64; the round-1 rule picked 32 there and cut 228 k of 524 k buckets in two).  Only when the buckets
  // alone cannot fill the chip twice (2 waves/SIMD x 1024 SIMDs x 64 lanes = 131 k lanes per round) are items made
  // shorter on purpose.  Skewed inputs (equal scalars, narrow top windows) still get cut at CH.
  const double mean_len = (double)n / (double)p.nb;
  uint32_t ch = 16;
  while (ch < 512 && (double)ch < mean_len + 5.0 * std::sqrt(mean_len)) ch <<= 1;
  while (ch > 16 && (size_t)p.W * p.nb + ((size_t)p.W * n) / ch < 262144) ch >>= 1;
  if (const char* e = std::getenv("MSM_AMD_CH")) {
    const int v = std::atoi(e);
    if (v >= 16 && v <= 512 && (v & (v - 1)) == 0) ch = (uint32_t)v;
  }
  p.CH = ch;
  p.red_L = (p.lb + 1) / 2;
  p.red_H = p.lb - p.red_L;
  p.red_group = kReduceGroup;
  p.total_buckets = (size_t)p.W * p.nb;
  p.total_segs = (size_t)p.W * reduce_scratch_elems(p.lb);   // scratch elements of each of the two sum families
  p.max_items = p.total_buckets + ((size_t)p.W * n) / ch + 1;
  p.partial_count = (size_t)p.W * (p.lb + 1);
  return p;
}

// Geometry of the window reduction alone (stage entry point sum_reduction).
Plan make_reduce_plan(uint32_t lb, uint32_t W) {
  Plan p{};
  p.c = lb + 1;   // only used to space bit positions in host_combine (one window at a time)
  p.W = W;
  p.lb = lb;
  p.nb = 1u << lb;
  p.red_L = (lb + 1) / 2;
  p.red_H = lb - p.red_L;
  p.red_group = kReduceGroup;
  p.total_buckets = (size_t)p.W * p.nb;
  p.total_segs = (size_t)p.W * reduce_scratch_elems(lb);
  p.partial_count = (size_t)p.W * (lb + 1);
  return p;
}

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

// Normalise to z = R mod p (or the canonical identity (1,1,0) in Montgomery form).
Jacobian normalise(const Jacobian& p) { return h64::store(h64::normalise(h64::load(p))); }

// E' -> E for a Jacobian point (Plan::on_iso): x = 4 x', y = 8 y' is Z <- Z / 2.  The identity (Z = 0) stays.
Jacobian iso_to_e(const Jacobian& q) {
  static const h64::Fe half = h64::inv(h64::dbl(h64::one()));
  h64::Jac j = h64::load(q);
  j.z = h64::mul(j.z, half);
  return h64::store(j);
}

// Window value  W_w = partial[w][lb] + sum_k 2^k * partial[w][k]  (total; bit sums of the column sums for k < L, of the
// row sums -- already offset by L -- for L <= k < lb; see k_reduce.hip) and the final Horner sum_w 2^(c*w) W_w, fused
// into ONE pass over bit positions: term partial[w][k] sits at bit c*w + k, the total at bit c*w.
// Replaces sum_reduction_final + final_accumulation.rs:19-39.
Jacobian host_combine(const Jacobian* partial, const Plan& p) {
  const uint32_t top = p.c * (p.W - 1) + p.lb;   // highest bit position in use
  // 4 x 64-bit host arithmetic (host_fq64.h): this pass is the whole CPU tail of an MSM
  h64::Jac acc = h64::identity();
  for (int pos = (int)top; pos >= 0; --pos) {
    acc = h64::jdouble(acc);
    // the terms at this bit: partial[w][k] with c w + k = pos and k < lb, and the window total partial[w][lb] at k = 0.
    // Production plans have lb = c - 1 (one window per position); tiny windows keep lb >= kSegLog > c - 1, where the
    // upper bit sums of window w share positions with window w + 1
    for (uint32_t w = std::min((uint32_t)pos / p.c, p.W - 1);; --w) {
      const uint32_t k = (uint32_t)pos - p.c * w;
      if (k > p.lb) break;
      const Jacobian* pw = partial + (size_t)w * (p.lb + 1);
      if (k == 0) acc = h64::jadd(acc, h64::load(pw[p.lb]));
      if (k < p.lb) acc = h64::jadd(acc, h64::load(pw[k]));
      if (w == 0) break;
    }
  }
  return h64::store(acc);
}

int set_kernel_attributes(msm_amd_ctx* ctx) {
  const char* failed = nullptr;
  if (sort_set_attributes(&failed) || reduce_set_attributes(&failed))
    return fail(ctx, MSM_AMD_FUNCTION_ERROR, std::string("hipFuncSetAttribute(") + (failed ? failed : "?") + ")");
  return MSM_AMD_OK;
}

// Events and page-locked room for partial_count points of ext_bytes each (+ the record of the plan counters).
int slot_prepare(msm_amd_ctx* ctx, InstanceSlot& s, size_t partial_count, size_t ext_bytes) {
  if (!s.has_events) {
    for (int i = 0; i < EV_COUNT; ++i) HIP_TRY(ctx, hipEventCreate(&s.ev[i]));
    s.has_events = true;
  }
  if (partial_count > s.h_partial_cap || ext_bytes != s.ext_bytes) {
    if (int rc = quiesce_for_allocation(ctx, "a page-locked result slot")) return rc;
    if (s.h_partial) HIP_TRY(ctx, hipHostFree(s.h_partial));
    s.h_partial = nullptr;
    s.h_partial_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&s.h_partial, (partial_count + 1) * ext_bytes, hipHostMallocDefault));
    s.h_partial_cap = partial_count;
    s.ext_bytes = ext_bytes;
  }
  return MSM_AMD_OK;
}

// ONE instance submitted while nothing else is in flight (what a blocking gpu_msm_h2c call is) runs on ONE stream:
// the front / accumulate / reduce split exists to overlap neighbouring instances, and with no neighbour its three
// cross-stream event hand-offs are pure latency -- 29 + 28 + 18 us of GPU idle time inside a 742 us call at 2^18
// points (profiles/r02_lone_call_2p18_timeline.txt).
bool lone_call(const msm_amd_ctx* ctx, size_t n_inst) {
  if (n_inst != 1 || !ctx->lone_single_stream) return false;
  for (const Batch& b : ctx->batches)
    if (b.active) return false;
  return true;
}
hipStream_t front_stream_of(const msm_amd_ctx* ctx, bool lone) {
  return (lone || !ctx->overlap_front) ? ctx->stream : ctx->front_stream;
}

// Bring inputs to the native device layout (scalars 32 B LE; affine 64 B Montgomery LE), on stream st.
// On return *scalars_native / *points_native point to device memory valid until the next call.
int convert_scalars(msm_amd_ctx* ctx, Workspace& w, hipStream_t st, int scalar_layout, const void* d_scalars, size_t n,
                    const u256** scalars_native, int* scalars_mont) {
  switch (scalar_layout) {
    case MSM_AMD_SCALAR_MONT_LE:
      *scalars_native = (const u256*)d_scalars;
      *scalars_mont = 1;
      break;
    case MSM_AMD_SCALAR_CANON_LE:
      *scalars_native = (const u256*)d_scalars;
      *scalars_mont = 0;
      break;
    case MSM_AMD_SCALAR_CANON_BE32: {
      int rc = ensure(ctx, w.conv_scalars, n * 32);
      if (rc) return rc;
      launch_be32_to_le(st, (const uint32_t*)d_scalars, n, (uint32_t*)w.conv_scalars.p);
      *scalars_native = (const u256*)w.conv_scalars.p;
      *scalars_mont = 0;
      break;
    }
    default:
      return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  }
  HIP_TRY(ctx, hipGetLastError());
  return MSM_AMD_OK;
}

int convert_points(msm_amd_ctx* ctx, Workspace& w, hipStream_t st, int point_layout, const void* d_points, size_t n,
                   const Affine** points_native) {
  switch (point_layout) {
    case MSM_AMD_POINT_PREPARED:   // already in the internal packed form (msm_amd_bases_*): nothing to convert
      *points_native = nullptr;
      break;
    case MSM_AMD_POINT_H2C_AFFINE:
      *points_native = (const Affine*)d_points;
      break;
    case MSM_AMD_POINT_ARK_PROJECTIVE: {
      int rc = ensure(ctx, w.conv_points, n * sizeof(Affine));
      if (rc) return rc;
      launch_projective_to_affine(st, (const Jacobian*)d_points, (uint32_t)n, (Affine*)w.conv_points.p);
      *points_native = (const Affine*)w.conv_points.p;
      break;
    }
    case MSM_AMD_POINT_ARK_AFFINE: {
      int rc = ensure(ctx, w.conv_points, n * sizeof(Affine));
      if (rc) return rc;
      launch_ark_affine_to_affine(st, (const uint8_t*)d_points, (uint32_t)n, (Affine*)w.conv_points.p);
      *points_native = (const Affine*)w.conv_points.p;
      break;
    }
    case MSM_AMD_POINT_JAC_BE32: {
      int rc = ensure(ctx, w.conv_tmp, n * sizeof(Jacobian));
      if (rc) return rc;
      rc = ensure(ctx, w.conv_points, n * sizeof(Affine));
      if (rc) return rc;
      launch_be32_to_le(st, (const uint32_t*)d_points, n * 3, (uint32_t*)w.conv_tmp.p);
      launch_projective_to_affine(st, (const Jacobian*)w.conv_tmp.p, (uint32_t)n, (Affine*)w.conv_points.p);
      *points_native = (const Affine*)w.conv_points.p;
      break;
    }
    default:
      return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown point layout");
  }
  HIP_TRY(ctx, hipGetLastError());
  return MSM_AMD_OK;
}

size_t scalar_bytes(int) { return 32; }
size_t point_bytes(int layout) {
  switch (layout) {
    case MSM_AMD_POINT_H2C_AFFINE: return 64;
    case MSM_AMD_POINT_PREPARED: return sizeof(AffPacked);
    case MSM_AMD_POINT_TABLES: return sizeof(AffPacked);
    case MSM_AMD_POINT_ARK_PROJECTIVE: return 96;
    case MSM_AMD_POINT_ARK_AFFINE: return 72;
    case MSM_AMD_POINT_JAC_BE32: return 96;
  }
  return 0;
}

// Room for the window reduction of plan p in workspace w: the two scratch families S, T (internal points) and the
// partial points (external points).
int reduce_buffers(msm_amd_ctx* ctx, Workspace& w, const Plan& p, size_t internal_bytes, size_t ext_bytes) {
  int rc;
  if ((rc = ensure(ctx, w.S, p.total_segs * internal_bytes))) return rc;
  if ((rc = ensure(ctx, w.T, p.total_segs * internal_bytes))) return rc;
  return ensure(ctx, w.partial, p.partial_count * ext_bytes);
}

// ---- handles: H = msm_amd_tables (ctx->live_tables), msm_amd_g2_tables (ctx->live_g2_tables), msm_amd_ntt_domain
// (ctx->live_ntt), msm_amd_fr_matrix (ctx->live_fr_mat) or msm_amd_poseidon_params (ctx->live_poseidon).  ctx->mu is held by
// the caller, as for every helper here.
template <class H>
const H* find_handle(const std::vector<H*>& live, const void* handle) {
  for (const H* t : live)
    if ((const void*)t == handle) return t;
  return nullptr;
}

// window_size 0 = `auto_c`; the window and the number of windows of a table over n points
int tables_geometry(msm_amd_ctx* ctx, size_t n, uint32_t window_size, uint32_t auto_c, uint32_t* c, uint32_t* W) {
  *c = window_size ? window_size : auto_c;
  if (*c < 4 || *c > 21) return fail(ctx, MSM_AMD_INPUT_ERROR, "table window_size must be 0 (auto) or 4..21");
  *W = kModulusBits / *c + 1;
  if ((size_t)*W * n > 0x7FFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "windows * n must stay below 2^31");
  return MSM_AMD_OK;
}

// The tail of a build: `bytes` of device memory (`memory` names it in messages), the build kernel (`launch(d_mem)` on
// ctx->stream), a bounded wait (for `build`) and the new handle in `live`; the caller fills in what its kind adds to
// DeviceHandle.
template <class H, class Launch>
int handle_build_tail(msm_amd_ctx* ctx, std::vector<H*>& live, size_t bytes, const std::string& memory,
                      const std::string& build, Launch&& launch, H** out) {
  void* d_mem = nullptr;
  if (int qrc = quiesce_for_allocation(ctx, memory.c_str())) return qrc;
  HIP_TRY(ctx, hipMalloc(&d_mem, bytes));
  launch(d_mem);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && sync_stream_bounded(ctx, ctx->stream, build.c_str())) {
    ctx->graveyard.push_back(d_mem);   // the build may still be running: released when the ctx is idle
    return MSM_AMD_PIPELINE_ERROR;
  }
  if (e != hipSuccess) {
    (void)hipFree(d_mem);
    HIP_TRY(ctx, e);
  }
  H* h = new H();
  h->d_mem = d_mem, h->bytes = bytes;
  live.push_back(h);
  *out = h;
  return MSM_AMD_OK;
}

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

template <class H>
int handle_free(msm_amd_ctx* ctx, std::vector<H*>& live, H* handle, const char* not_a_handle) {
  auto it = std::find(live.begin(), live.end(), handle);
  if (it == live.end()) return fail(ctx, MSM_AMD_INPUT_ERROR, not_a_handle);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  live.erase(it);
  if (drain_or_mark_stalled(ctx)) (void)hipFree(handle->d_mem);
  else ctx->graveyard.push_back(handle->d_mem);   // hipFree would wait for the device without bound
  delete handle;
  return MSM_AMD_OK;
}

// msm_amd_destroy: handles the caller did not free
template <class H>
void handle_release_all(std::vector<H*>& live) {
  for (H* h : live) {
    (void)hipFree(h->d_mem);
    delete h;
  }
  live.clear();
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

bool scalar_layout_ok(int scalar_layout) {
  return scalar_layout >= MSM_AMD_SCALAR_MONT_LE && scalar_layout <= MSM_AMD_SCALAR_CANON_BE32;
}

// ms between two recorded events (0 if either cannot be read)
float event_span(hipEvent_t a, hipEvent_t b) {
  float t = 0;
  if (hipEventElapsedTime(&t, a, b) != hipSuccess) {
    (void)hipGetLastError();
    t = 0;
  }
  return t;
}

// Row / column sums of the window reduction for a LONE call: with no neighbouring instance to fill the machine, the
// 15-addition chains of the pipelined setting (one lane per 16 buckets: 35 k lanes at 2^18 points, 7.7 k in the second
// level at 2^20) are pure latency.  launch_reduce then takes, level by level, the smallest group (>= this minimum) whose
// outputs still fit the lanes one launch can have resident; a further level costs one launch (~5 us), one addition
// in a chain about 6 us.
uint32_t pick_reduce_group(const Plan&) {
  if (const char* e = std::getenv("MSM_AMD_REDUCE_GROUP")) return (uint32_t)std::atoi(e);
  return kReduceGroupMin;
}

// The buffers of the scalar front end (digits, sort, work-item planning) of one MSM in workspace w, grown to plan p,
// and the SortBuffers that name them (redo_list stays null: experiments only, see enqueue_msm).  p.n = sorted entries
// per window (the points, or W_digits * points with tables).
int front_buffers(msm_amd_ctx* ctx, Workspace& w, const Plan& p, SortBuffers* sb) {
  int rc;
  if ((rc = ensure(ctx, w.digits, (size_t)p.W * p.n * (p.wide_digits ? sizeof(uint32_t) : sizeof(uint16_t))))) return rc;
  if ((rc = ensure(ctx, w.coarse_cnt, (size_t)p.W * p.Q * (1u << p.hb) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.region_start, (size_t)p.W * ((1u << p.hb) + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.tmp_idx, (size_t)p.W * p.n * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.tmp_fine, (size_t)p.W * p.n * sizeof(uint16_t)))) return rc;
  if (p.mb) {
    if ((rc = ensure(ctx, w.tmp_idx2, (size_t)p.W * p.n * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, w.tmp_fine2, (size_t)p.W * p.n * sizeof(uint16_t)))) return rc;
    if ((rc = ensure(ctx, w.mid_cnt, ((size_t)p.W << p.hb) * p.Q2 * (1u << p.mb) * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, w.region_start2, (size_t)p.W * ((1u << (p.hb + p.mb)) + 1) * sizeof(uint32_t)))) return rc;
  }
  if ((rc = ensure(ctx, w.bsize, p.total_buckets * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.bstart, p.total_buckets * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.istart, p.total_buckets * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.win_items, (1024 + 2 * 1024) * sizeof(uint32_t)))) return rc;   // + tile_sums (<= 1024 tiles)
  if ((rc = ensure(ctx, w.size_bins, (size_t)(p.CH + 1) * ((p.total_buckets + p.front_threads - 1) / p.front_threads) *
                                         sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.sorted, (size_t)p.W * p.n * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.order, p.max_items * sizeof(uint2)))) return rc;
  if ((rc = ensure(ctx, w.multi_list, p.max_items * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, w.counters, sizeof(PlanCounters)))) return rc;
  *sb = SortBuffers{};
  sb->digits = w.digits.p;
  sb->coarse_cnt = (uint32_t*)w.coarse_cnt.p;
  sb->region_start = (uint32_t*)w.region_start.p;
  sb->tmp_idx = (uint32_t*)w.tmp_idx.p;
  sb->tmp_fine = (uint16_t*)w.tmp_fine.p;
  sb->tmp_idx2 = (uint32_t*)w.tmp_idx2.p;
  sb->tmp_fine2 = (uint16_t*)w.tmp_fine2.p;
  sb->mid_cnt = (uint32_t*)w.mid_cnt.p;
  sb->region_start2 = (uint32_t*)w.region_start2.p;
  sb->bucket_size = (uint32_t*)w.bsize.p;
  sb->bucket_start = (uint32_t*)w.bstart.p;
  sb->item_start = (uint32_t*)w.istart.p;
  sb->win_items = (uint32_t*)w.win_items.p;
  sb->tile_sums = (uint2*)((uint32_t*)w.win_items.p + 1024);   // second half of the same small buffer
  sb->size_bins = (uint32_t*)w.size_bins.p;
  sb->sorted = (uint32_t*)w.sorted.p;
  sb->order = (uint2*)w.order.p;
  sb->multi_list = (uint32_t*)w.multi_list.p;
  sb->counters = (PlanCounters*)w.counters.p;
  return MSM_AMD_OK;
}

// The plan of one instance: make_plan and what depends on whether the instance has the machine to itself.
Plan instance_plan(size_t n, uint32_t c, uint32_t table_windows, bool lone, WidthBound width = WidthBound{}) {
  Plan p = make_plan(n, c, table_windows, width);
  if (lone) p.red_group = pick_reduce_group(p);   // (pipelined small instances: 2^16 -6 %, 2^18 +3 % -- not taken)
  p.rb_threads = lone ? 0u : 64u;                 // one wave per bit-subset sum beside a resident accumulate grid (k_reduce.hip)
  // the tile-staged scatter (1024-thread workgroups, 60 VGPRs, 64 KB of LDS) is for a sort that has the machine to
  // itself; beside a resident accumulate grid it is slower than the plain scatter (4 x 2^22 points: 6.15 vs 5.65 ms per MSM)
  if (!lone && !std::getenv("MSM_AMD_TILED")) p.tiled = 0;
  return p;
}

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

// The group-independent front end of one instance on stream fs: scalar conversion, the group's base conversion (inside
// the convert span), digits, sort and work-item planning, with their stage events; then the main stream waits for it.
// rs: the stream the instance will reduce on.
int enqueue_front(msm_amd_ctx* ctx, Workspace& w, InstanceSlot& slot, const Plan& p, const SortBuffers& sb, hipStream_t fs,
                  hipStream_t rs, bool lone, int scalar_layout, const void* d_scalars, const PointStages& g) {
  hipStream_t st = ctx->stream;
  if (w.acc_pending && (fs != st || lone)) {   // the previous accumulate in this workspace still reads its plan ...
    HIP_TRY(ctx, hipStreamWaitEvent(fs, w.acc_done, 0));
  }
  if (w.reduce_pending && (fs != rs || lone)) {   // ... and so does its combine pass (on whichever reduce stream
    HIP_TRY(ctx, hipStreamWaitEvent(fs, w.reduce_done, 0));   // the previous user of the workspace had)
  }
  w.acc_pending = false;
  if (ctx->upload_pending) {   // scalars staged by the entry point (stage_upload): order them before this front end
    if (fs != ctx->upload_stream) {
      HIP_TRY(ctx, hipEventRecord(ctx->upload_done, ctx->upload_stream));
      HIP_TRY(ctx, hipStreamWaitEvent(fs, ctx->upload_done, 0));
      ctx->upload_stream = fs;   // later point ranges of the same call run their front ends on this stream too
    }
  }
  HIP_TRY(ctx, hipEventRecord(slot.ev[EV_START], fs));
  const u256* sc = nullptr;
  int sc_mont = 0, rc;
  if ((rc = convert_scalars(ctx, w, fs, scalar_layout, d_scalars, p.n_scalars, &sc, &sc_mont))) return rc;
  if ((rc = g.convert_bases(fs))) return rc;
  HIP_TRY(ctx, hipEventRecord(slot.ev[EV_CONVERT], fs));
  if (p.fused_front) launch_digits_hist(fs, p, sc, sc_mont, sb); else launch_digits(fs, p, sc, sc_mont, sb.digits, sb.counters);
  HIP_TRY(ctx, hipEventRecord(slot.ev[EV_DIGITS], fs));
  launch_sort(fs, p, sb, p.fused_front);
  HIP_TRY(ctx, hipEventRecord(slot.ev[EV_SORT], fs));
  if (fs != st) {
    HIP_TRY(ctx, hipEventRecord(w.front_done, fs));
    HIP_TRY(ctx, hipStreamWaitEvent(st, w.front_done, 0));
  }
  return MSM_AMD_OK;
}

// The point-valued half of one instance: accumulate on the main stream; combine, window reduction and the copy of the
// partial points and the plan counters into the slot on stream rs.
int enqueue_points(msm_amd_ctx* ctx, Workspace& w, InstanceSlot& slot, const Plan& p, const SortBuffers& sb, hipStream_t rs,
                   const PointStages& g) {
  hipStream_t st = ctx->stream;
  // the bucket matrix is NOT cleared: a bucket without points gets no work item and is never written; the window
  // reduction reads bucket_size and takes such a slot as the identity (the reference relies on Metal's zero-filled
  // fresh buffers instead, msm.rs:154-156)
  if (w.reduce_pending) {   // the previous user of this workspace may still be reducing its buckets
    if (rs != st) HIP_TRY(ctx, hipStreamWaitEvent(st, w.reduce_done, 0));
    w.reduce_pending = false;
  }
  g.accumulate(st, sb, slot.ev[EV_ACC_K0], slot.ev[EV_ACC_K1]);
  if (w.acc_done) {
    HIP_TRY(ctx, hipEventRecord(w.acc_done, st));
    w.acc_pending = true;
  }
  // combine (split buckets) + window reduction + copy: off the main stream, which goes straight to the next
  // accumulate.  front(i+2) reuses this workspace's plan buffers, which combine still reads: it waits for
  // reduce_done as well (see the top of enqueue_front).
  if (rs != st) HIP_TRY(ctx, hipStreamWaitEvent(rs, w.acc_done, 0));
  g.combine(rs, sb);
  if (int rc = reduce_buffers(ctx, w, p, g.internal_bytes, g.ext_bytes)) return rc;
  g.reduce(rs);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(slot.h_partial, w.partial.p, p.partial_count * g.ext_bytes, hipMemcpyDeviceToHost, rs));
  HIP_TRY(ctx, hipMemcpyAsync(slot.h_partial + slot.h_partial_cap * g.ext_bytes, w.counters.p, sizeof(PlanCounters),
                              hipMemcpyDeviceToHost, rs));
  HIP_TRY(ctx, hipEventRecord(slot.ev[EV_REDUCE], rs));
  if (w.reduce_done) {
    HIP_TRY(ctx, hipEventRecord(w.reduce_done, rs));
    w.reduce_pending = true;
  }
  HIP_TRY(ctx, hipGetLastError());
  return MSM_AMD_OK;
}

// Enqueue one whole instance of plan p, G1 or G2, in workspace w; the partial points and the plan counters land in
// slot.h_partial after slot.ev[EV_REDUCE].  Four streams (front, main, two alternating reduce streams), kWorkspaces
// workspaces (consecutive instances take consecutive workspaces):
//   front  : conversion, digits, sort, planning of instance i -- needs the workspace's previous accumulate and
//            reduction done; runs while instance i-1 accumulates and i-2 reduces
//   main   : accumulate of instance i                         -- needs front(i)
//   reduce : combine + window reduction + copy of instance i  -- needs main(i)
// A lone instance has all three on the main stream (lone_call).
int enqueue_instance(msm_amd_ctx* ctx, Workspace& w, InstanceSlot& slot, const Plan& p, bool lone, int scalar_layout,
                     const void* d_scalars, const PointStages& g) {
  int rc;
  if ((rc = slot_prepare(ctx, slot, p.partial_count, g.ext_bytes))) return rc;
  SortBuffers sb{};
  if ((rc = front_buffers(ctx, w, p, &sb))) return rc;
  if (ctx->acc_variant == 4) {   // experiments build: the hand-allocated kernel's redo pass
    if ((rc = ensure(ctx, w.redo_list, p.max_items * sizeof(uint32_t)))) return rc;
    sb.redo_list = (uint32_t*)w.redo_list.p;
  }
  if (g.bases_bytes && (rc = ensure(ctx, w.bases29, g.bases_bytes))) return rc;
  if ((rc = ensure(ctx, w.buckets, p.total_buckets * g.internal_bytes))) return rc;
  if ((rc = ensure(ctx, w.item_partials, p.max_items * g.internal_bytes))) return rc;
  hipStream_t fs = front_stream_of(ctx, lone);
  hipStream_t rs = (lone || !ctx->overlap_reduce)
                       ? ctx->stream
                       : ctx->reduce_streams[ctx->alt_reduce ? ctx->seq++ % kReduceStreams : 0];
  if ((rc = enqueue_front(ctx, w, slot, p, sb, fs, rs, lone, scalar_layout, d_scalars, g))) return rc;
  return enqueue_points(ctx, w, slot, p, sb, rs, g);
}

// One G1 instance: d_points holds n points of point_layout, prepared bases or, with MSM_AMD_POINT_TABLES, is the handle
// of msm_amd_tables_build*.
int enqueue_msm(msm_amd_ctx* ctx, Workspace& w, InstanceSlot& slot, int scalar_layout, int point_layout, const void* d_scalars,
                const void* d_points, size_t n, Plan* plan_out, bool lone) {
  const msm_amd_tables* tb = nullptr;
  if (point_layout == MSM_AMD_POINT_TABLES) {
    tb = find_handle(ctx->live_tables, d_points);
    if (!tb) return fail(ctx, MSM_AMD_INPUT_ERROR, "not a table handle of this ctx");
    if (n != tb->n) return fail(ctx, MSM_AMD_INPUT_ERROR, "n differs from the number of points the tables hold");
  }
  const WidthBound width = ctx->bound;
  const uint32_t c = tb ? tb->c : (ctx->forced_window ? ctx->forced_window : auto_window_bounded(n, width.width(), lone));
  Plan p = instance_plan(n, c, tb ? tb->W : 0, lone, width);
  const bool prepared = point_layout == MSM_AMD_POINT_PREPARED || tb != nullptr;
  AffPacked* const fill = prepared ? nullptr : ctx->convert_into;   // bases cache fill: convert straight into the entry
  // Bases that are not kept (no prepared array, table or cache entry) are not converted: accumulate gathers the external
  // records in place -- the caller's device array (H2C_AFFINE) or the Affine array convert_points wrote into the
  // workspace (ark layouts, BE32) -- and the instance runs on E'.  Host slices of msm_amd_msm_batch stay on the
  // conversion kernel (their staging set is re-used after EV_DIGITS), and so do the experiments build's variant kernels.
  const bool in_place = !prepared && !fill && !ctx->staging_points && (ctx->acc_variant == 0 || ctx->acc_variant == 1);
  p.on_iso = in_place;
  *plan_out = p;
#if defined(MSM_AMD_EXPERIMENTS)
  // variant 8: bases converted inside this call go into WIDE records (128 B: x, y, -y as limbs)
  const bool wide = !prepared && !fill && ctx->acc_variant == 8;
  const size_t base_record = wide ? sizeof(AffWide) : sizeof(AffPacked);
#else
  const bool wide = false;
  const size_t base_record = sizeof(AffPacked);
#endif
  PointStages g;
  g.bases_bytes = (prepared || fill || in_place) ? 0 : p.n * base_record;
  const Affine* ext_bases = nullptr;   // in_place: set by convert_bases, read by accumulate (enqueued after it)
  g.internal_bytes = sizeof(PtI);
  g.ext_bytes = sizeof(Jacobian);
  g.convert_bases = [&](hipStream_t fs) -> int {
    const Affine* pts = nullptr;
    if (int rc = convert_points(ctx, w, fs, prepared ? MSM_AMD_POINT_PREPARED : point_layout, d_points, p.n_scalars, &pts))
      return rc;
#if defined(MSM_AMD_EXPERIMENTS)
    if (wide) launch_convert_bases_wide(fs, pts, p.n, (AffWide*)w.bases29.p);
#endif
    ext_bases = pts;
    if (!prepared && !wide && !in_place)   // external 8 x u32 -> packed internal domain
      launch_convert_bases(fs, pts, p.n, fill ? fill : (AffPacked*)w.bases29.p);
    return MSM_AMD_OK;
  };
  g.accumulate = [&](hipStream_t st, const SortBuffers& sb, hipEvent_t before, hipEvent_t after) {
    const void* bases = tb ? tb->d_mem
                           : (prepared ? d_points : (fill ? (const void*)fill : (in_place ? (const void*)ext_bases : w.bases29.p)));
    launch_accumulate(st, p, bases, wide ? 1 : 0, sb, (PtI*)w.buckets.p, (PtI*)w.item_partials.p, ctx->acc_variant,
                      ctx->acc_lds, before, after);
  };
  g.combine = [&](hipStream_t st, const SortBuffers& sb) { launch_combine(st, p, sb, (PtI*)w.buckets.p, (PtI*)w.item_partials.p); };
  g.reduce = [&](hipStream_t st) {
    launch_reduce(st, p, (const PtI*)w.buckets.p, (const uint32_t*)w.bsize.p, (PtI*)w.S.p, (PtI*)w.T.p, (Jacobian*)w.partial.p);
  };
  return enqueue_instance(ctx, w, slot, p, lone, scalar_layout, d_scalars, g);
}

void accumulate_timings(msm_amd_ctx* ctx, InstanceSlot& s, const Plan& p, float final_ms, size_t n_inst) {
  auto span = [&](int a, int b) { return event_span(s.ev[a], s.ev[b]); };
  float ms[EV_COUNT] = {0};
  ms[EV_CONVERT] = span(EV_START, EV_CONVERT);
  ms[EV_DIGITS] = span(EV_CONVERT, EV_DIGITS);
  ms[EV_SORT] = span(EV_DIGITS, EV_SORT);
  ms[EV_ACC] = span(EV_ACC_S, EV_ACC);
  ms[EV_REDUCE] = span(EV_RED_S, EV_REDUCE);
  msm_amd_timings& T = ctx->timings;
  const float inv = 1.0f / (float)n_inst;
  T.convert_ms += ms[EV_CONVERT] * inv;
  T.digits_ms += ms[EV_DIGITS] * inv;
  T.sort_ms += ms[EV_SORT] * inv;
  T.accumulate_ms += ms[EV_ACC] * inv;
  T.reduce_ms += ms[EV_REDUCE] * inv;
  T.accumulate_kernel_ms += span(EV_ACC_K0, EV_ACC_K1) * inv;
  T.final_ms += final_ms * inv;
  T.total_gpu_ms += (ms[EV_CONVERT] + ms[EV_DIGITS] + ms[EV_SORT] + ms[EV_ACC] + ms[EV_REDUCE]) * inv;
  T.n = p.n_scalars;
  T.window_size = p.c;
  T.num_windows = p.W_digits;
  T.reserved = (uint32_t)n_inst;
  T.reserved2[0] = (float)s.counters().total_items;   // work items (= lanes with work) of the last instance's accumulate grid
  T.reserved2[1] = ctx->after_sort_state;
  T.reserved2[2] = ctx->after_sort_lead_ms;
}

// Batch of MSMs with device-resident inputs, in two halves so that callers can pipeline batches:
//   submit_batch_device  enqueues every kernel of every instance (four streams, see enqueue_msm) and returns
//   wait_batch           finishes each instance on the host as soon as its partial points have landed (the host
//                        Horner pass of instance i overlaps the GPU work of i+1.. and of later batches)
// lone_hint: -1 = decide here (one instance, nothing in flight), 0 / 1 = the caller (run_batch_host, which submits
// the instances of ITS batch one by one and has already put the upload waits on a stream) decided
int submit_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                        const void* const* d_scalars, const void* const* d_points, const size_t* n, void* out_host,
                        int* ticket, int lone_hint = -1) {
  if (!ctx || !d_scalars || !d_points || !n || !out_host || !ticket || n_inst == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "null argument or empty batch");
  if (point_bytes(point_layout) == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown point layout");
  for (size_t i = 0; i < n_inst; ++i) {
    if (n[i] == 0 || n[i] > 0x7FFFFFFFull || !d_scalars[i] || !d_points[i])
      return fail(ctx, MSM_AMD_INPUT_ERROR, "instance with n == 0, n >= 2^31 or null pointer");
  }
  if (int rc = recover_if_stalled(ctx)) return rc;
  int id = -1;
  for (int b = 0; b < kMaxBatches; ++b)
    if (!ctx->batches[b].active) {
      id = b;
      break;
    }
  if (id < 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "too many batches in flight: wait for one first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool lone = lone_hint < 0 ? lone_call(ctx, n_inst) : lone_hint != 0;
  Batch& B = ctx->batches[id];
  if (B.slots.size() < n_inst) B.slots.resize(n_inst);
  B.plans.assign(n_inst, Plan{});
  B.ws_index.assign(n_inst, 0);
  B.first_index.assign(n_inst, 0);
  if (ctx->range_first)
    for (size_t i = 0; i < n_inst; ++i) B.first_index[i] = ctx->range_first[ctx->range_at + i];
  B.lone = lone;
  B.out = out_host;
  B.n_inst = n_inst;
  if (ctx->last_waited == id) ctx->last_waited = -1;   // its record is about to be overwritten
  for (size_t i = 0; i < n_inst; ++i) {
    B.ws_index[i] = ctx->next_ws;
    Workspace& w = ctx->ws[ctx->next_ws];
    ctx->next_ws = (ctx->next_ws + 1) % kWorkspaces;
    int rc = enqueue_msm(ctx, w, B.slots[i], scalar_layout, point_layout, d_scalars[i], d_points[i], n[i], &B.plans[i],
                         lone);
    if (rc) {   // nothing of a failed submit stays in flight (or the ctx is marked stalled); the slot was never active
      (void)drain_or_mark_stalled(ctx);
      return rc;
    }
  }
  B.active = true;
  *ticket = id;
  return MSM_AMD_OK;
}

// Host threads for the CPU tail (window Horner pass + normalisation, ~0.11 ms per instance) of one batch.  Batches of
// small MSMs are bound by it: 40 x 2^12 points take 0.16 ms per MSM on one thread, of which 0.11 ms is this pass and
// 0.05 ms the enqueue.  One thread per 4 instances, at most 4 and at most half of the cores; MSM_AMD_FINISH_THREADS
// overrides (1 = the calling thread only).
unsigned finish_threads(size_t n_inst) {
  if (const char* e = std::getenv("MSM_AMD_FINISH_THREADS")) return (unsigned)std::max(1, std::atoi(e));
  const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
  return (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)4, n_inst / 4, (size_t)hw / 2}));
}

// wait_event on s.ev[EV_REDUCE] ran into the ctx's bound: the ctx is stalled, and the error names `what` and the last
// stage event of the instance the device did get to.
// msm_amd_last_error of a bounded call that met records beyond its bound
std::string width_violation_message(const Plan& p, size_t records, size_t instances, size_t instance, size_t n_inst,
                                    size_t index) {
  std::string m = std::to_string(records) + " record(s) with a magnitude of 2^" + std::to_string(p.bits) + " or more (" +
                  (p.sign ? "signed" : "unsigned") + " bound of " + std::to_string(p.bits) + " bits)";
  if (n_inst > 1)
    m += " in " + std::to_string(instances) + " of " + std::to_string(n_inst) + " instances; one of them: instance " +
         std::to_string(instance) + ", index " + std::to_string(index);
  else
    m += "; one of them: index " + std::to_string(index);
  return m + "; the output was not written";
}

int wait_timed_out(msm_amd_ctx* ctx, const InstanceSlot& s, const std::string& what, const char* tail = "") {
  ctx->stalled = true;
  int reached = -1;
  for (int e = 0; e < EV_COUNT; ++e) {
    if (hipEventQuery(s.ev[e]) == hipSuccess) reached = e;
  }
  (void)hipGetLastError();
  return fail(ctx, MSM_AMD_PIPELINE_ERROR,
              "timed out after " + std::to_string(ctx->wait_timeout_ms) + " ms waiting for event 'reduce' of " + what +
                  "; last event reached: " + (reached < 0 ? "none" : kEventNames[reached]) + tail);
}

// `internal`: the caller is one of the library's blocking entry points, which cannot hand the ticket back to its own
// caller -- on a timed-out wait the batch is marked abandoned (released by recover_if_stalled once the device is idle).
// Through msm_amd_wait_batch the ticket stays valid and the caller may wait again.
int wait_batch(msm_amd_ctx* ctx, int ticket, bool internal = true) {
  if (!ctx || ticket < 0 || ticket >= kMaxBatches || !ctx->batches[ticket].active || ctx->batches[ticket].abandoned)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown batch ticket");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Batch& B = ctx->batches[ticket];
  ctx->timings = msm_amd_timings{};
  struct Done {
    hipError_t err = hipSuccess;
    float final_ms = 0;
    uint32_t viol = 0, viol_index = 0;   // a bounded instance: records beyond the bound, the lowest index of one
    Jacobian res;                        // ... whose result waits here until every instance of the batch has kept its bound
  };
  bool bounded = false;   // an instance whose bound a record can exceed: nothing is written before all are checked
  for (size_t i = 0; i < B.n_inst; ++i) bounded = bounded || B.plans[i].bits != 0;
  std::vector<Done> done(B.n_inst);
  const uint32_t timeout_ms = ctx->wait_timeout_ms;
  // instance i: wait for its partial sums, Horner pass, result; instances are independent, each writes its own slot
  auto finish_from = [&](size_t first, size_t stride, bool set_device) {
    if (set_device && hipSetDevice(ctx->device) != hipSuccess) {
      for (size_t i = first; i < B.n_inst; i += stride) done[i].err = hipErrorInvalidDevice;
      return;
    }
    for (size_t i = first; i < B.n_inst; i += stride) {
      InstanceSlot& s = B.slots[i];
      done[i].err = wait_event(s.ev[EV_REDUCE], timeout_ms);
      if (done[i].err != hipSuccess) {
        if (done[i].err == hipErrorNotReady) {   // the later instances of this thread are behind the same stall
          for (size_t k = i + stride; k < B.n_inst; k += stride) done[k].err = hipErrorNotReady;
          return;
        }
        continue;
      }
      const auto t0 = std::chrono::steady_clock::now();
      // the one place every consumer of a G1 instance goes through: a sum computed on E' comes back to E here
      const Jacobian sum = host_combine((const Jacobian*)s.h_partial, B.plans[i]);
      const Jacobian res = normalise(B.plans[i].on_iso ? iso_to_e(sum) : sum);
      done[i].final_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (bounded) {
        const PlanCounters pc = s.counters();
        if (B.plans[i].bits) done[i].viol = pc.viol[0], done[i].viol_index = ~pc.viol[1];
        done[i].res = res;
      } else {
        std::memcpy((uint8_t*)B.out + i * 96, &res, 96);
      }
    }
  };
  const unsigned T = std::min<size_t>(finish_threads(B.n_inst), B.n_inst);
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(finish_from, (size_t)t, (size_t)T, true);
  finish_from(0, T, false);
  for (std::thread& th : pool) th.join();
  for (size_t i = 0; i < B.n_inst; ++i) {
    if (done[i].err == hipErrorNotReady) {   // the bound of the wait was reached: the work is still in flight
      if (internal) B.abandoned = true;
      return wait_timed_out(ctx, B.slots[i],
                            "instance " + std::to_string(i) + " of " + std::to_string(B.n_inst) + " (ticket " +
                                std::to_string(ticket) + ")",
                            internal ? "" : "; the ticket stays valid");
    }
    if (done[i].err != hipSuccess) {   // release the ticket on every exit: a failed wait must not block later submits
      if (!drain_or_mark_stalled(ctx)) B.abandoned = true;
      else B.active = false;
      return fail(ctx, MSM_AMD_PIPELINE_ERROR, std::string("hipEventQuery: ") + hipGetErrorString(done[i].err));
    }
    accumulate_timings(ctx, B.slots[i], B.plans[i], done[i].final_ms, B.n_inst);
  }
  B.active = false;
  if (bounded) {   // the GPU work is done either way; a violated bound leaves the output as it was
    for (size_t i = 0; i < B.n_inst; ++i)
      if (done[i].viol) {
        size_t records = 0, instances = 0;
        for (size_t k = 0; k < B.n_inst; ++k) records += done[k].viol, instances += done[k].viol ? 1 : 0;
        reap_graveyard(ctx);
        return fail(ctx, MSM_AMD_INPUT_ERROR, width_violation_message(B.plans[i], records, instances, i, B.n_inst,
                                                                       B.first_index[i] + done[i].viol_index));
      }
    for (size_t i = 0; i < B.n_inst; ++i) std::memcpy((uint8_t*)B.out + i * 96, &done[i].res, 96);
  }
  ctx->last_waited = ticket;
  reap_graveyard(ctx);
  return MSM_AMD_OK;
}

// Is this host pointer page-locked (msm_amd_host_register, hipHostMalloc, hipHostRegister)?
bool host_pinned(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// Pageable uploads of one range overlap the kernels of the previous range only if the runtime's staged copy does not
// serialise with the device.  Measured on this image: the system runtime (HIP 7.2) overlaps them (2^22 host points:
// 14.0 -> 9.6 ms with 4 ranges); the HIP 7.0 runtime bundled with the PyTorch wheel -- which the process binds to when
// torch is imported first, as in bench.py -- does not (14.0 -> 14.9 ms).  Page-locked buffers overlap on both.
bool pageable_uploads_overlap() {
  static const bool ok = [] {
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return v >= 70200000;
  }();
  return ok;
}

void stager_worker(Stager* S, int part) {
  uint64_t seen = 0;
  for (;;) {
    const uint8_t* src;
    uint8_t* dst;
    size_t bytes;
    // chunks of one upload follow each other within ~100 us: spin that long before going to sleep on the condvar
    for (int spin = 0; spin < 20000 && S->generation.load(std::memory_order_acquire) == seen; ++spin) __builtin_ia32_pause();
    {
      std::unique_lock<std::mutex> lk(S->m);
      S->wake.wait(lk, [&] { return S->quit || S->generation.load() != seen; });
      if (S->quit) return;
      seen = S->generation.load();
      src = S->src;
      dst = S->dst;
      bytes = S->bytes;
    }
    const size_t parts = (size_t)S->n_helpers + 1, lo = bytes * part / parts, hi = bytes * (part + 1) / parts;
    std::memcpy(dst + lo, src + lo, hi - lo);
    {
      std::lock_guard<std::mutex> lk(S->m);
      if (--S->pending == 0) S->finished.notify_one();
    }
  }
}

int stager_prepare(msm_amd_ctx* ctx) {
  Stager& S = ctx->stager;
  if (S.ready) return MSM_AMD_OK;
  if (int rc = quiesce_for_allocation(ctx, "the page-locked staging ring")) return rc;
  for (int k = 0; k < Stager::kSlots; ++k) {
    HIP_TRY(ctx, hipHostMalloc(&S.slot[k], Stager::kChunk, hipHostMallocDefault));
    HIP_TRY(ctx, hipEventCreateWithFlags(&S.sent[k], hipEventDisableTiming));
  }
  if (const char* e = std::getenv("MSM_AMD_STAGE_HELPERS")) S.n_helpers = std::max(1, std::min(Stager::kMaxHelpers, std::atoi(e)));
  for (int h = 1; h <= S.n_helpers; ++h) S.helpers.emplace_back(stager_worker, &S, h);
  S.ready = true;
  return MSM_AMD_OK;
}

void stager_shutdown(msm_amd_ctx* ctx) {
  Stager& S = ctx->stager;
  if (!S.ready) return;
  {
    std::lock_guard<std::mutex> lk(S.m);
    S.quit = true;
  }
  S.wake.notify_all();
  for (std::thread& t : S.helpers) t.join();
  S.helpers.clear();
  for (int k = 0; k < Stager::kSlots; ++k) {
    if (S.sent[k]) (void)hipEventDestroy(S.sent[k]);
    if (S.slot[k]) (void)hipHostFree(S.slot[k]);
    S.sent[k] = nullptr;
    S.slot[k] = nullptr;
  }
  S.ready = false;
}

// Should a pageable upload of this size go through the ring?  By default where the runtime's own staged copy does not
// overlap kernels (HIP < 7.2); MSM_AMD_STAGED_UPLOAD=0 / 1 overrides.
bool stage_pageable(msm_amd_ctx* ctx, const void* src, size_t bytes) {
  if (bytes < 2 * Stager::kChunk) return false;
  if (ctx->staged_uploads < 0) {
    const char* e = std::getenv("MSM_AMD_STAGED_UPLOAD");
    ctx->staged_uploads = e ? (std::atoi(e) != 0) : (pageable_uploads_overlap() ? 0 : 1);
  }
  return ctx->staged_uploads == 1 && !host_pinned(src);
}

// hipMemcpyAsync(dst, src, bytes, H2D, stream) for a pageable src, through the ring.  Returns when the last chunk has
// been handed to the DMA engine (the caller's buffer is no longer needed), not when it has arrived.
int staged_upload(msm_amd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t stream) {
  int rc;
  if ((rc = stager_prepare(ctx))) return rc;
  Stager& S = ctx->stager;
  for (size_t off = 0; off < bytes; off += Stager::kChunk) {
    const size_t len = std::min(Stager::kChunk, bytes - off);
    const int k = S.next;
    S.next = (S.next + 1) % Stager::kSlots;
    if (S.busy[k]) {
      if (wait_event(S.sent[k], ctx->wait_timeout_ms) != hipSuccess)
        return fail(ctx, MSM_AMD_PIPELINE_ERROR, "timed out waiting for a staged upload chunk to leave its slot");
      S.busy[k] = false;
    }
    {
      std::lock_guard<std::mutex> lk(S.m);
      S.src = (const uint8_t*)h_src + off;
      S.dst = (uint8_t*)S.slot[k];
      S.bytes = len;
      S.pending = S.n_helpers;
      ++S.generation;
    }
    S.wake.notify_all();
    std::memcpy(S.slot[k], (const uint8_t*)h_src + off, len / ((size_t)S.n_helpers + 1));   // part 0 on this thread
    {
      std::unique_lock<std::mutex> lk(S.m);
      S.finished.wait(lk, [&] { return S.pending == 0; });
    }
    HIP_TRY(ctx, hipMemcpyAsync((uint8_t*)d_dst + off, S.slot[k], len, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(S.sent[k], stream));
    S.busy[k] = true;
  }
  return MSM_AMD_OK;
}

// A LONE call of many points runs as ONE PIPELINED BATCH of sub-instances over point ranges (the algebra of the
// reference's GPU + CPU split, msm.rs:385-419: the MSM of a union of point ranges is the sum of the MSMs).  Alone, an
// instance is a serial chain upload -> conversion / digits / sort -> accumulate -> reduction; as a batch, the front end
// (and, from host buffers, the upload) of range k + 1 overlaps the accumulate kernel of range k.  Costs: one window
// reduction and one host Horner pass per range (overlapped, except the last) and a final addition of `parts` points.
// Thresholds measured on MI355X (profiles/r02_lone_call_split.txt); MSM_AMD_SPLIT=<parts> forces a count, 1 disables.
unsigned split_parts(const msm_amd_ctx* ctx, int point_layout, size_t n, bool host_buffers, const void* scalars = nullptr,
                     const void* points = nullptr) {
  if (point_layout == MSM_AMD_POINT_TABLES || !lone_call(ctx, 1)) return 1;
  unsigned parts = 1;
  if (const char* e = std::getenv("MSM_AMD_SPLIT")) {
    parts = (unsigned)std::max(1, std::min(8, std::atoi(e)));
  } else {
    const uint32_t l = floor_log2(n);
    if (host_buffers) {   // the upload overlaps too
      const bool dev_points = point_layout == MSM_AMD_POINT_PREPARED;
      const bool pinned = scalars && host_pinned(scalars) && (dev_points || (points && host_pinned(points)));
      if (pinned || pageable_uploads_overlap()) parts = l >= 22 ? 8 : (l >= 20 ? 4 : (l >= 19 ? 2 : 1));
    } else {
      parts = l >= 24 ? 8 : (l == 23 ? 4 : 1);
    }
  }
  while (parts > 1 && n / parts < 4096) parts >>= 1;
  return parts;
}

// ---- bases cache ------------------------------------------------------------------------------------------------
inline uint64_t mix64(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
inline uint64_t hash_record(uint64_t h, const uint8_t* rec, size_t pb) {
  for (size_t o = 0; o + 8 <= pb; o += 8) {
    uint64_t v;
    std::memcpy(&v, rec + o, 8);
    h = mix64(h, v);
  }
  return h;
}
size_t cache_phases(size_t n) { return std::max<size_t>(1, n / 1024); }
uint64_t hash_phase(const void* host, size_t n, size_t pb, size_t S, size_t phase) {
  uint64_t h = 0x243F6A8885A308D3ull ^ (uint64_t)n ^ ((uint64_t)phase << 40);
  const uint8_t* base = (const uint8_t*)host;
  for (size_t i = phase; i < n; i += S) h = hash_record(h, base + i * pb, pb);
  return h;
}

// Full verification: the array as kCacheChunks contiguous slices, each hashed sequentially, the slices spread over a
// few short-lived threads (a 64 MiB array: ~1.5 ms on four threads against ~12 ms on one).
constexpr size_t kCacheChunks = 64;
void hash_chunks(const void* host, size_t n, size_t pb, uint64_t* out) {
  const uint8_t* base = (const uint8_t*)host;
  auto one = [&](size_t c) {
    const size_t lo = n * c / kCacheChunks, hi = n * (c + 1) / kCacheChunks;
    uint64_t h = 0x13198A2E03707344ull ^ (uint64_t)n ^ ((uint64_t)c << 48);
    for (size_t i = lo; i < hi; ++i) h = hash_record(h, base + i * pb, pb);
    out[c] = h;
  };
  const size_t T = n * pb >= ((size_t)4 << 20) ? 4 : 1;
  std::vector<std::thread> th;
  try {
    for (size_t t = 1; t < T; ++t)
      th.emplace_back([&, t] { for (size_t c = t; c < kCacheChunks; c += T) one(c); });
  } catch (...) {
    for (std::thread& x : th) x.join();
    th.clear();
    for (size_t c = 0; c < kCacheChunks; ++c) one(c);
    return;
  }
  const size_t started = th.size() + 1;
  for (size_t c = 0; c < kCacheChunks; c += started) one(c);
  for (std::thread& x : th) x.join();
}

void bases_cache_drop(msm_amd_ctx* ctx, size_t k) {
  BasesCacheEntry& e = ctx->bases_cache[k];
  if (e.d_prepared) ctx->graveyard.push_back(e.d_prepared);   // hipFree waits for the whole device: later (reap_graveyard)
  ctx->bases_cache_bytes -= e.n * sizeof(AffPacked);
  ctx->bases_cache.erase(ctx->bases_cache.begin() + (long)k);
}

void bases_cache_clear(msm_amd_ctx* ctx) {
  while (!ctx->bases_cache.empty()) bases_cache_drop(ctx, ctx->bases_cache.size() - 1);
}

// Hit: the entry (checksums verified against the caller's memory).  A stale entry is dropped and counts as a miss.
BasesCacheEntry* bases_cache_lookup(msm_amd_ctx* ctx, const void* host, size_t n, int layout) {
  for (size_t k = 0; k < ctx->bases_cache.size(); ++k) {
    BasesCacheEntry& e = ctx->bases_cache[k];
    if (e.host != host || e.n != n || e.layout != layout) continue;
    const size_t pb = point_bytes(layout), S = e.phase_hash.size();
    bool same = hash_phase(host, n, pb, S, 0) == e.phase_hash[0];
    if (same && ctx->bases_cache_verify) {   // every record, every hit
      uint64_t now[kCacheChunks];
      hash_chunks(host, n, pb, now);
      same = std::memcmp(now, e.chunk_hash.data(), sizeof now) == 0;
    } else if (same && S > 1) {
      const uint32_t ph = e.next_phase;
      e.next_phase = ph + 1 >= S ? 1 : ph + 1;
      same = hash_phase(host, n, pb, S, ph) == e.phase_hash[ph];
    }
    if (!same) {
      if (e.last_use == ctx->bases_cache_call) return nullptr;   // in use by this very call: leave it, just do not hit
      ++ctx->bases_cache_invalidations;
      bases_cache_drop(ctx, k);
      return nullptr;
    }
    e.last_use = ctx->bases_cache_call;
    ++ctx->bases_cache_hits;
    return &e;
  }
  return nullptr;
}

// Start of a host-slice call: room on the device for those of its arrays that have no entry yet (least recently used
// entries that this call will not hit make way).  The ctx is idle here or is waited for, bounded; an array that gets
// no room runs uncached.
void bases_cache_reserve(msm_amd_ctx* ctx, size_t n_inst, const void* const* points, const size_t* n, int layout) {
  for (const msm_amd_ctx::CacheReserve& r : ctx->cache_reserve) ctx->graveyard.push_back(r.d);   // an earlier call's leftovers
  ctx->cache_reserve.clear();
  if (!ctx->bases_cache_budget) return;
  auto has_key = [&](size_t j) {
    for (const BasesCacheEntry& e : ctx->bases_cache)
      if (e.host == points[j] && e.n == n[j] && e.layout == layout) return true;
    for (const msm_amd_ctx::CacheReserve& r : ctx->cache_reserve)
      if (r.host == points[j] && r.n == n[j] && r.layout == layout) return true;
    return false;
  };
  for (size_t j = 0; j < n_inst; ++j)   // what this call is about to hit stays
    for (BasesCacheEntry& e : ctx->bases_cache)
      if (e.host == points[j] && e.n == n[j] && e.layout == layout) e.wanted_by = ctx->bases_cache_call;
  bool idle = false;
  size_t reserved_bytes = 0;
  for (size_t j = 0; j < n_inst; ++j) {
    if (!points[j] || has_key(j)) continue;
    const size_t bytes = n[j] * sizeof(AffPacked);
    if (bytes > ctx->bases_cache_budget) continue;
    bool room = true;
    while (ctx->bases_cache_bytes + reserved_bytes + bytes > ctx->bases_cache_budget) {
      size_t victim = ctx->bases_cache.size();
      for (size_t k = 0; k < ctx->bases_cache.size(); ++k)
        if (ctx->bases_cache[k].last_use != ctx->bases_cache_call && ctx->bases_cache[k].wanted_by != ctx->bases_cache_call &&
            (victim == ctx->bases_cache.size() || ctx->bases_cache[k].last_use < ctx->bases_cache[victim].last_use))
          victim = k;
      if (victim == ctx->bases_cache.size()) {
        room = false;
        break;
      }
      bases_cache_drop(ctx, victim);
    }
    if (!room) continue;
    if (!idle) {
      if (!streams_idle(ctx) && !drain_streams_bounded(ctx)) return;   // busy past the bound: this call runs uncached
      idle = true;
    }
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    ctx->cache_reserve.push_back({points[j], n[j], layout, d});
    reserved_bytes += bytes;
  }
}

// Miss: a new entry on the room bases_cache_reserve made for it, or nullptr -- the instance then runs uncached.
BasesCacheEntry* bases_cache_insert(msm_amd_ctx* ctx, const void* host, size_t n, int layout) {
  const size_t bytes = n * sizeof(AffPacked);
  for (size_t k = 0; k < ctx->bases_cache.size(); ++k)   // a stale twin the lookup had to leave alone
    if (ctx->bases_cache[k].host == host && ctx->bases_cache[k].n == n && ctx->bases_cache[k].layout == layout)
      return nullptr;
  BasesCacheEntry e;
  e.host = host;
  e.n = n;
  e.layout = layout;
  for (size_t k = 0; k < ctx->cache_reserve.size(); ++k)
    if (ctx->cache_reserve[k].host == host && ctx->cache_reserve[k].n == n && ctx->cache_reserve[k].layout == layout) {
      e.d_prepared = ctx->cache_reserve[k].d;
      ctx->cache_reserve.erase(ctx->cache_reserve.begin() + (long)k);
      break;
    }
  if (!e.d_prepared) return nullptr;
  const size_t pb = point_bytes(layout), S = cache_phases(n);
  e.phase_hash.assign(S, 0);
  for (size_t ph = 0; ph < S; ++ph) e.phase_hash[ph] = 0x243F6A8885A308D3ull ^ (uint64_t)n ^ ((uint64_t)ph << 40);
  const uint8_t* base = (const uint8_t*)host;
  size_t ph = 0;
  for (size_t i = 0; i < n; ++i) {   // one sequential pass fills every phase
    e.phase_hash[ph] = hash_record(e.phase_hash[ph], base + i * pb, pb);
    if (++ph == S) ph = 0;
  }
  e.chunk_hash.assign(kCacheChunks, 0);
  hash_chunks(host, n, pb, e.chunk_hash.data());
  e.last_use = ctx->bases_cache_call;
  ctx->bases_cache_bytes += bytes;
  ++ctx->bases_cache_misses;
  ctx->bases_cache.push_back(std::move(e));
  return &ctx->bases_cache.back();
}

int run_batch_host(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst, const void* const* scalars,
                   const void* const* points, const size_t* n, void* out);
int run_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                     const void* const* d_scalars, const void* const* d_points, const size_t* n, void* out_host);

int run_split(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* scalars, const void* points, size_t n,
              unsigned parts, void* out, bool host_buffers) {
  const size_t sb = scalar_bytes(scalar_layout), pb = point_bytes(point_layout);
  std::vector<const void*> sp(parts), pp(parts);
  std::vector<size_t> nn(parts);
  std::vector<uint8_t> outs((size_t)parts * 96);
  std::vector<size_t> first(parts);
  for (unsigned k = 0; k < parts; ++k) {
    const size_t b = n * k / parts, e = n * (k + 1) / parts;
    first[k] = b;
    sp[k] = (const uint8_t*)scalars + sb * b;
    pp[k] = (const uint8_t*)points + pb * b;
    nn[k] = e - b;
  }
  int rc;
  ctx->range_first = first.data(), ctx->range_at = 0;
  struct Reset {
    msm_amd_ctx* c;
    ~Reset() { c->range_first = nullptr, c->range_at = 0; }
  } reset{ctx};
  if (host_buffers) {
    rc = run_batch_host(ctx, scalar_layout, point_layout, parts, sp.data(), pp.data(), nn.data(), outs.data());
  } else {
    int ticket = -1;
    rc = submit_batch_device(ctx, scalar_layout, point_layout, parts, sp.data(), pp.data(), nn.data(), outs.data(),
                             &ticket, 0);
    if (!rc) rc = wait_batch(ctx, ticket);
  }
  if (rc) return rc;
  h64::Jac acc = h64::identity();
  for (unsigned k = 0; k < parts; ++k) {
    h64::Jac p;
    std::memcpy(&p, outs.data() + (size_t)k * 96, 96);
    acc = h64::jadd(acc, p);
  }
  const h64::Jac res = h64::normalise(acc);
  std::memcpy(out, &res, 96);
  // stage spans of the call = sums over its ranges (wait_batch / run_batch_host report per-instance averages)
  msm_amd_timings& T = ctx->timings;
  const float P = (float)parts;
  T.convert_ms *= P; T.digits_ms *= P; T.sort_ms *= P; T.accumulate_ms *= P; T.accumulate_kernel_ms *= P;
  T.reduce_ms *= P; T.final_ms *= P; T.total_gpu_ms *= P;
  T.n = (uint32_t)n;
  T.reserved = parts;
  return MSM_AMD_OK;
}

int run_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                     const void* const* d_scalars, const void* const* d_points, const size_t* n, void* out_host) {
  if (n_inst == 1 && ctx && d_scalars && d_points && n && d_scalars[0] && d_points[0]) {
    const unsigned parts = split_parts(ctx, point_layout, n[0], false);
    if (parts > 1)
      return run_split(ctx, scalar_layout, point_layout, d_scalars[0], d_points[0], n[0], parts, out_host, false);
  }
  int ticket = -1;
  int rc = submit_batch_device(ctx, scalar_layout, point_layout, n_inst, d_scalars, d_points, n, out_host, &ticket);
  if (rc) return rc;
  return wait_batch(ctx, ticket);
}

int upload_one(msm_amd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, bool ring = true) {
  if (ring && stage_pageable(ctx, h_src, bytes)) return staged_upload(ctx, d_dst, h_src, bytes, ctx->copy_stream);
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
  return MSM_AMD_OK;
}

void uploader_main(msm_amd_ctx* ctx) {
  Uploader& U = ctx->uploader;
  (void)hipSetDevice(ctx->device);
  std::string my_error;
  tl_error_sink = &my_error;
  for (;;) {
    UploadJob j;
    {
      std::unique_lock<std::mutex> lk(U.m);
      U.cv.wait(lk, [&] { return U.quit || U.has_job; });
      if (U.quit) return;
      j = U.job;
      U.has_job = false;
    }
    int rc = MSM_AMD_OK;
    hipError_t e = hipSuccess;
    if (j.wait_for) e = hipStreamWaitEvent(ctx->copy_stream, j.wait_for, 0);
    if (e == hipSuccess) rc = upload_one(ctx, j.d_scalars, j.h_scalars, j.scalar_bytes);
    if (e == hipSuccess && !rc && j.point_bytes) rc = upload_one(ctx, j.d_points, j.h_points, j.point_bytes);
    if (e == hipSuccess && !rc) e = hipEventRecord(j.done, ctx->copy_stream);
    {
      std::lock_guard<std::mutex> lk(U.m);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        rc = MSM_AMD_PIPELINE_ERROR;
        U.error = std::string("upload: ") + hipGetErrorString(e);
      } else if (rc) {
        U.error = my_error;
      }
      U.status = rc;
      U.busy = false;
    }
    U.cv_idle.notify_all();
  }
}

void uploader_dispatch(msm_amd_ctx* ctx, const UploadJob& j) {
  Uploader& U = ctx->uploader;
  if (!U.started) {
    U.th = std::thread(uploader_main, ctx);
    U.started = true;
  }
  {
    std::lock_guard<std::mutex> lk(U.m);
    U.job = j;
    U.has_job = true;
    U.busy = true;
  }
  U.cv.notify_one();
}

int uploader_await(msm_amd_ctx* ctx) {   // the dispatched job has been enqueued completely (or has failed)
  Uploader& U = ctx->uploader;
  if (!U.started) return MSM_AMD_OK;
  std::unique_lock<std::mutex> lk(U.m);
  U.cv_idle.wait(lk, [&] { return !U.busy; });
  const int rc = U.status;
  U.status = MSM_AMD_OK;
  if (rc) ctx->last_error = U.error;
  return rc;
}

void uploader_shutdown(msm_amd_ctx* ctx) {
  Uploader& U = ctx->uploader;
  if (!U.started) return;
  (void)uploader_await(ctx);
  {
    std::lock_guard<std::mutex> lk(U.m);
    U.quit = true;
  }
  U.cv.notify_all();
  U.th.join();
  U.started = false;
  U.quit = false;
}

// Host-buffer variant: stage inputs into device scratch, then run the device path per instance.
int run_batch_host(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst, const void* const* scalars,
                   const void* const* points, const size_t* n, void* out) {
  if (!ctx || !scalars || !points || !n || !out || n_inst == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "null argument or empty batch");
  const size_t pb = point_bytes(point_layout);
  if (pb == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown point layout");
  // prepared bases / window tables live on the device already: points[i] is the device pointer / table handle and
  // only the scalars (32 bytes per point instead of 96) cross PCIe -- the repeated-SRS case
  const bool dev_points = point_layout == MSM_AMD_POINT_PREPARED || point_layout == MSM_AMD_POINT_TABLES;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = recover_if_stalled(ctx)) return rc;
  if (n_inst == 1 && scalars[0] && points[0] && n[0]) {   // a lone call of many points: pipelined point ranges
    const unsigned parts = split_parts(ctx, point_layout, n[0], true, scalars[0], points[0]);
    if (parts > 1) return run_split(ctx, scalar_layout, point_layout, scalars[0], points[0], n[0], parts, out, true);
  }
  for (size_t i = 0; i < n_inst; ++i) {
    if (n[i] == 0 || !scalars[i] || !points[i]) return fail(ctx, MSM_AMD_INPUT_ERROR, "n == 0 or null pointer");
    if (point_layout == MSM_AMD_POINT_PREPARED) {   // must really be device memory: a host array here would fault
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, points[i]) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(ctx, MSM_AMD_INPUT_ERROR,
                    "MSM_AMD_POINT_PREPARED takes the device array written by msm_amd_bases_upload / "
                    "msm_amd_bases_prepare_device, not a host buffer");
      }
    }
  }
  // Two staging sets and up to three instances in flight.  Uploads run on their own stream (DMA for buffers the
  // caller registered, msm_amd_host_register; the runtime's staged copy, which blocks this thread, for pageable
  // memory): the upload of instance i waits -- on the GPU, not on the host -- until the front end of instance
  // i - 2 has read the staging set (its EV_DIGITS event: conversion, convert_bases and digits are done), and the
  // front-end stream of instance i waits for the upload.  The host only blocks to collect instance i - 3.
  constexpr size_t kInflight = 3;
  static_assert(kInflight <= (size_t)kMaxBatches, "one ticket per instance in flight");
  std::vector<int> tickets(n_inst, -1);
  msm_amd_timings avg{};
  size_t collected = 0;
  auto collect = [&](size_t i) {   // wait for instance i and fold its stage times into the running average
    int rc = wait_batch(ctx, tickets[i]);
    tickets[i] = -1;
    if (rc) return rc;
    const msm_amd_timings& T = ctx->timings;
    const float a = (float)collected / (float)(collected + 1), b = 1.0f / (float)(collected + 1);
    msm_amd_timings k = T;
    k.convert_ms = avg.convert_ms * a + T.convert_ms * b;
    k.digits_ms = avg.digits_ms * a + T.digits_ms * b;
    k.sort_ms = avg.sort_ms * a + T.sort_ms * b;
    k.accumulate_ms = avg.accumulate_ms * a + T.accumulate_ms * b;
    k.accumulate_kernel_ms = avg.accumulate_kernel_ms * a + T.accumulate_kernel_ms * b;
    k.reduce_ms = avg.reduce_ms * a + T.reduce_ms * b;
    k.final_ms = avg.final_ms * a + T.final_ms * b;
    k.total_gpu_ms = avg.total_gpu_ms * a + T.total_gpu_ms * b;
    k.reserved = (uint32_t)(++collected);
    avg = k;
    return (int)MSM_AMD_OK;
  };
  auto bail = [&](int rc) {   // error exit: nothing of this call may stay in flight or hold a ticket
    ctx->convert_into = nullptr;
    for (BasesCacheEntry& c : ctx->bases_cache)   // an entry filled by this call may never have been written: no hits
      if (c.last_use == ctx->bases_cache_call) c.host = nullptr;
    if (ctx->stalled) {       // ... unless the device is not answering: leave the rest to recover_if_stalled
      for (int t : tickets)
        if (t >= 0) ctx->batches[t].abandoned = true;
      return rc;
    }
    if (!drain_or_mark_stalled(ctx)) {
      for (int t : tickets)
        if (t >= 0) ctx->batches[t].abandoned = true;
      return rc;
    }
    for (int t : tickets)
      if (t >= 0) ctx->batches[t].active = false;
    return rc;
  };
  {   // staging buffers are sized once, before anything is in flight (growing one would free memory in use)
    size_t max_n = 0;
    for (size_t i = 0; i < n_inst; ++i) max_n = std::max(max_n, n[i]);
    int rc;
    for (DeviceBuf* b : {&ctx->scratch_b, &ctx->scratch_b2})
      if ((rc = ensure(ctx, *b, max_n * scalar_bytes(scalar_layout)))) return rc;
    if (!dev_points)
      for (DeviceBuf* b : {&ctx->scratch_c, &ctx->scratch_c2})
        if ((rc = ensure(ctx, *b, max_n * pb))) return rc;
  }
  const bool lone = lone_call(ctx, n_inst);
  hipStream_t fs = front_stream_of(ctx, lone);
  const bool use_cache = ctx->bases_cache_budget != 0 && !dev_points;
  if (use_cache) bases_cache_reserve(ctx, n_inst, points, n, point_layout);
  // bases cache (opt-in): a hit replaces the 64..96 B per point upload and the conversion by the resident converted
  // copy; a miss uploads as usual and converts straight into the new entry (the reference re-uploads and re-converts
  // the bases on every call, msm.rs:152-153; its callers pass the same SRS slice again and again,
  // benches/msm_benchmark.rs:116-121)
  std::vector<const void*> cached(n_inst, nullptr);
  std::vector<AffPacked*> fill(n_inst, nullptr);
  // upload of instance j on the helper thread (uploader_main), decided and dispatched by this one
  auto dispatch = [&](size_t j) -> int {
    if (use_cache) {
      if (BasesCacheEntry* e = bases_cache_lookup(ctx, points[j], n[j], point_layout)) cached[j] = e->d_prepared;
      else if (BasesCacheEntry* f = bases_cache_insert(ctx, points[j], n[j], point_layout)) fill[j] = (AffPacked*)f->d_prepared;
    }
    UploadJob job;
    job.d_scalars = ((j & 1) ? ctx->scratch_b2 : ctx->scratch_b).p;
    job.h_scalars = scalars[j];
    job.scalar_bytes = n[j] * scalar_bytes(scalar_layout);
    if (!dev_points && !cached[j]) {
      job.d_points = ((j & 1) ? ctx->scratch_c2 : ctx->scratch_c).p;
      job.h_points = points[j];
      job.point_bytes = n[j] * pb;
    }
    // the staging set's previous reader is instance j - 2: its front end has read the set once its digits are done
    if (j >= 2) job.wait_for = ctx->batches[tickets[j - 2]].slots[0].ev[EV_DIGITS];
    job.done = ctx->uploaded[j & 1];
    if (n_inst > 1) {
      uploader_dispatch(ctx, job);
      return (int)MSM_AMD_OK;
    }
    // ONE instance: nothing to overlap the upload with -- the plain copy on this thread is the shortest path (the
    // helper thread's hand-offs and the ring cost a lone 2^18 call 0.2 ms, measured)
    int rc = upload_one(ctx, job.d_scalars, job.h_scalars, job.scalar_bytes, false);
    if (!rc && job.point_bytes) rc = upload_one(ctx, job.d_points, job.h_points, job.point_bytes, false);
    if (!rc && hipEventRecord(job.done, ctx->copy_stream) != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(ctx, MSM_AMD_PIPELINE_ERROR, "hipEventRecord(uploaded)");
    }
    return rc;
  };
  auto bail_upload = [&](int rc) {   // the helper may still be reading the caller's buffers
    (void)uploader_await(ctx);
    return bail(rc);
  };
  if (int rc0 = dispatch(0)) return bail(rc0);
  for (size_t i = 0; i < n_inst; ++i) {
    int rc;
    if (i >= kInflight && (rc = collect(i - kInflight))) return bail_upload(rc);
    if (n_inst > 1 && (rc = uploader_await(ctx))) return bail(rc);   // upload i is enqueued, uploaded[i & 1] recorded
    // upload i + 1 goes on while this thread enqueues the kernels of instance i (its staging set was last read by
    // instance i - 1, submitted in the previous iteration)
    if (i + 1 < n_inst) (void)dispatch(i + 1);
    const hipError_t e = hipStreamWaitEvent(fs, ctx->uploaded[i & 1], 0);
    if (e != hipSuccess) return bail_upload(fail(ctx, MSM_AMD_PIPELINE_ERROR, hipGetErrorString(e)));
    const void* ds = ((i & 1) ? ctx->scratch_b2 : ctx->scratch_b).p;
    const void* dp = dev_points ? points[i] : (cached[i] ? cached[i] : ((i & 1) ? ctx->scratch_c2 : ctx->scratch_c).p);
    int ticket = -1;
    ctx->convert_into = fill[i];
    ctx->staging_points = !dev_points && !cached[i];
    ctx->range_at = i;
    rc = submit_batch_device(ctx, scalar_layout, cached[i] ? (int)MSM_AMD_POINT_PREPARED : point_layout, 1, &ds, &dp, &n[i],
                             (uint8_t*)out + i * 96, &ticket, lone ? 1 : 0);
    ctx->convert_into = nullptr;
    ctx->staging_points = false;
    if (rc) return bail_upload(rc);
    tickets[i] = ticket;
  }
  for (size_t i = n_inst > kInflight ? n_inst - kInflight : 0; i < n_inst; ++i) {
    int rc = collect(i);
    if (rc) return bail(rc);
  }
  ctx->timings = avg;
  return MSM_AMD_OK;
}

// Host -> device copy of a single-instance entry point's inputs into ctx scratch.  The copy goes on the stream a lone
// call's front end uses (no cross-stream hand-off in the common case); enqueue_msm orders it before the front end
// if that ends up on another stream -- a call of many points becomes pipelined point ranges (run_split), whose front
// ends run on the front stream.  With pageable memory the runtime's staged copy blocks the host and hid the missing
// edge; with page-locked scalars (msm_amd_host_register) digits_kernel could read the scratch before the DMA landed.
int stage_upload(msm_amd_ctx* ctx, void* dst, const void* src, size_t bytes) {
  hipStream_t up = front_stream_of(ctx, lone_call(ctx, 1));
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, up));
  ctx->upload_stream = up;
  ctx->upload_pending = true;
  return MSM_AMD_OK;
}

// The instances submitted while this lives are planned with `width` (ctx->mu is held by the entry point).
struct BoundScope {
  msm_amd_ctx* ctx;
  BoundScope(msm_amd_ctx* c, uint32_t bits, int sign) : ctx(c) { ctx->bound.bits = bits, ctx->bound.sign = (uint32_t)sign; }
  ~BoundScope() { ctx->bound = WidthBound{}; }
};

// the (bits, sign) of a bounded entry point `who`
int bound_args(msm_amd_ctx* ctx, const char* who, uint32_t bits, int sign) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (const char* why = width_bound_check(bits, sign)) return fail(ctx, MSM_AMD_INPUT_ERROR, std::string(who) + ": " + why);
  return MSM_AMD_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

const char* msm_amd_version(void) {
#if defined(MSM_AMD_EXPERIMENTS)
  return "msm_amd 0.4 (gfx950) +experiments";
#else
  return "msm_amd 0.4 (gfx950)";
#endif
}

const char* msm_amd_strerror(int status) {
  switch (status) {
    case MSM_AMD_OK: return "ok";
    case MSM_AMD_DEVICE_NOT_FOUND: return "Couldn't find a HIP device (MetalError::DeviceNotFound)";
    case MSM_AMD_LIBRARY_ERROR: return "Couldn't load the gfx950 code object (MetalError::LibraryError)";
    case MSM_AMD_FUNCTION_ERROR: return "Couldn't set up a kernel function (MetalError::FunctionError)";
    case MSM_AMD_PIPELINE_ERROR: return "HIP launch/runtime failure (MetalError::PipelineError)";
    case MSM_AMD_INPUT_ERROR: return "Invalid input (MetalError::InputError)";
    case MSM_AMD_FILE_OPEN_ERROR: return "I/O error (HarnessError::FileOpenError)";
    case MSM_AMD_DESERIALIZATION_ERROR: return "Data in file is invalid or incomplete (HarnessError::DeserializationError)";
    case MSM_AMD_INVALID_DATA: return "Invalid data (HarnessError::InvalidData)";
  }
  return "unknown status";
}

const char* msm_amd_last_error(const msm_amd_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int msm_amd_init(int device, msm_amd_ctx** out) {
  if (!out) return MSM_AMD_INPUT_ERROR;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return MSM_AMD_DEVICE_NOT_FOUND;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) return MSM_AMD_DEVICE_NOT_FOUND;
  }
  if (device >= count) return MSM_AMD_DEVICE_NOT_FOUND;
  if (hipSetDevice(device) != hipSuccess) return MSM_AMD_DEVICE_NOT_FOUND;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MSM_AMD_DEVICE_NOT_FOUND;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    // the code object is built for gfx950 only: fail loudly instead of falling back
    std::fprintf(stderr, "msm_amd: device %d is %s, this library targets gfx950 (MI355X)\n", device,
                 prop.gcnArchName);
    return MSM_AMD_LIBRARY_ERROR;
  }
  msm_amd_ctx* ctx = new msm_amd_ctx();
  ctx->device = device;
  if (const char* e = std::getenv("MSM_AMD_OVERLAP_REDUCE")) ctx->overlap_reduce = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSM_AMD_OVERLAP_FRONT")) ctx->overlap_front = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSM_AMD_ALT_REDUCE")) ctx->alt_reduce = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSM_AMD_LONE_SINGLE_STREAM")) ctx->lone_single_stream = std::atoi(e) != 0;
  ctx->acc_variant = ctx->overlap_front ? 1 : 0;
  if (const char* e = std::getenv("MSM_AMD_LOW_OCC")) ctx->acc_variant = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("MSM_AMD_ACC_VARIANT")) ctx->acc_variant = std::atoi(e);
  if (const char* e = std::getenv("MSM_AMD_ACC_LDS")) ctx->acc_lds = (uint32_t)std::atoi(e);
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  // the short front-end / reduction kernels get priority over the long accumulate grid
  // CREATION ORDER MATTERS: HIP maps streams onto four hardware queues in creation order, so the fifth stream (copy,
  // idle in device-resident runs) shares the queue of the first (main).  With the reduce streams created last, one
  // of them shared the accumulate grid's queue and every second window reduction waited behind it: 760 -> 720 MSM/s
  // on the same box (profiles/r02_stream_creation_order_ab.txt).  The copy stream is best off on the main stream's
  // queue as well: on a reduce stream's queue the host-slice batches lose 4 %, on the front stream's 18 %.
  bool ok = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_least) == hipSuccess;
  for (int k = 0; ok && k < kReduceStreams; ++k)
    ok = hipStreamCreateWithPriority(&ctx->reduce_streams[k], hipStreamNonBlocking, prio_greatest) == hipSuccess;
  ok = ok &&
            hipStreamCreateWithPriority(&ctx->front_stream, hipStreamNonBlocking, prio_greatest) == hipSuccess &&
            hipStreamCreateWithPriority(&ctx->copy_stream, hipStreamNonBlocking, prio_greatest) == hipSuccess &&
            hipEventCreateWithFlags(&ctx->uploaded[0], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ctx->uploaded[1], hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ctx->upload_done, hipEventDisableTiming) == hipSuccess;
  ctx->wait_timeout_ms = default_wait_timeout_ms();
  if (const char* e = std::getenv("MSM_AMD_MUL_CHUNK")) {
    const size_t want = std::max<size_t>(1, (size_t)std::strtoull(e, nullptr, 10));
    ctx->mul_chunk = std::min<size_t>((want + kMulNormGroup - 1) / kMulNormGroup * kMulNormGroup, (size_t)1 << 24);
  }
  if (const char* e = std::getenv("MSM_AMD_NTT_TILE_LOG"))
    ctx->ntt_tile_log = (uint32_t)std::max(2, std::min((int)kNttTileLog, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_FR_TILE_LOG"))
    ctx->fr_tile_log = (uint32_t)std::max((int)kFrMinTileLog, std::min((int)kFrTileLog, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_FR_MAT_LONG"))
    ctx->fr_mat_long = (uint32_t)std::max((int)kFrMatMinLong, std::min((int)kFrMatMaxLong, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_FR_MAT_SIGNS")) ctx->fr_mat_signs = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSM_AMD_FR_MLE_CHUNK_LOG"))
    ctx->fr_mle_chunk_log = (uint32_t)std::max((int)kFrMleMinChunkLog, std::min((int)kFrMleMaxChunkLog, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_POSEIDON_TOP_LOG"))
    ctx->poseidon_top_log = (uint32_t)std::max(0, std::min((int)kPoseidonMaxTopLog, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_FR_MAT_SEG_LOG"))
    ctx->fr_mat_seg_log = (uint32_t)std::max((int)kFrMatMinSegLog, std::min((int)kFrMatMaxSegLog, std::atoi(e)));
  if (const char* e = std::getenv("MSM_AMD_BASES_CACHE_VERIFY")) ctx->bases_cache_verify = std::strcmp(e, "full") == 0;
  if (const char* e = std::getenv("MSM_AMD_BASES_CACHE_MB")) {
    ctx->bases_cache_budget = (size_t)std::strtoull(e, nullptr, 10) << 20;
    if (ctx->bases_cache_budget)   // switched on from OUTSIDE the calling code: say so, once per ctx
      std::fprintf(stderr,
                   "libmsm_amd: MSM_AMD_BASES_CACHE_MB=%s: host-slice entry points now reuse converted bases by (pointer, "
                   "n, layout); a hit is verified %s -- callers that change bases in place must call "
                   "msm_amd_bases_cache_invalidate\n",
                   e, ctx->bases_cache_verify ? "in full (every record)" : "by sampling (MSM_AMD_BASES_CACHE_VERIFY=full re-hashes every record)");
  }
  for (int k = 0; ok && k < kWorkspaces; ++k)
    ok = hipEventCreateWithFlags(&ctx->ws[k].front_done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&ctx->ws[k].acc_done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&ctx->ws[k].reduce_done, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    delete ctx;
    return MSM_AMD_PIPELINE_ERROR;
  }
  int rc = set_kernel_attributes(ctx);
  if (rc) {
    std::fprintf(stderr, "msm_amd: %s\n", ctx->last_error.c_str());
    (void)hipStreamDestroy(ctx->stream);
    for (hipStream_t rs : ctx->reduce_streams)
      if (rs) (void)hipStreamDestroy(rs);
    (void)hipStreamDestroy(ctx->front_stream);
    (void)hipStreamDestroy(ctx->copy_stream);
    (void)hipEventDestroy(ctx->uploaded[0]);
    (void)hipEventDestroy(ctx->uploaded[1]);
    (void)hipEventDestroy(ctx->upload_done);
    delete ctx;
    return rc;
  }
  *out = ctx;
  return MSM_AMD_OK;
}

int msm_amd_init_reusable(msm_amd_ctx** out) {
  if (!out) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(g_global_mu);
  if (!g_global_ctx) {
    int rc = msm_amd_init(-1, &g_global_ctx);
    if (rc) return rc;
  }
  *out = g_global_ctx;
  return MSM_AMD_OK;
}

int msm_amd_get_global(msm_amd_ctx** out) {
  if (!out) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(g_global_mu);
  if (!g_global_ctx) return MSM_AMD_INPUT_ERROR;
  *out = g_global_ctx;
  return MSM_AMD_OK;
}

// Teardown order: wait until the DEVICE is idle (every stream of the ctx, the copy stream included, and whatever the
// runtime still has queued: a profiler's own work), then events, then memory, then streams, every handle nulled.
// (Round 2 freed buffers and events stream by stream without ever synchronising the copy stream; under rocprofv3 a
// profiled 2^24-point run once stalled and once aborted AFTER its last kernel had completed, i.e. in here / at exit.)
void msm_amd_destroy(msm_amd_ctx* ctx) {
  if (!ctx) return;
  {
    std::lock_guard<std::mutex> g(g_global_mu);
    if (ctx == g_global_ctx) g_global_ctx = nullptr;
  }
  std::unique_lock<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  if (!drain_streams_bounded(ctx)) {
    // the device does not answer: freeing memory under work in flight would turn a stall into a fault.  Give the
    // device resources up (they go with the process) and release the host side only.
    std::fprintf(stderr, "msm_amd_destroy: device %d still busy after %u ms; leaking the ctx's device resources\n",
                 ctx->device, ctx->wait_timeout_ms);
    lk.unlock();
    return;
  }
  (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  auto kill_event = [](hipEvent_t& e) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  };
  auto kill_buf = [](DeviceBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  };
  auto kill_stream = [](hipStream_t& s) {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  };
  // 1. events
  auto kill_slot_events = [&](InstanceSlot& s) {
    if (s.has_events)
      for (int i = 0; i < EV_COUNT; ++i) kill_event(s.ev[i]);
    s.has_events = false;
  };
  for (Batch& B : ctx->batches)
    for (InstanceSlot& s : B.slots) kill_slot_events(s);
  for (int k = 0; k < kWorkspaces; ++k) {
    kill_event(ctx->ws[k].front_done);
    kill_event(ctx->ws[k].acc_done);
    kill_event(ctx->ws[k].reduce_done);
  }
  kill_slot_events(ctx->g2.slot);   // (g2.ws has no hand-off events)
  for (hipEvent_t& e : ctx->uploaded) kill_event(e);
  kill_event(ctx->upload_done);
  kill_event(ctx->after_sort_mark);
  uploader_shutdown(ctx);
  stager_shutdown(ctx);
  // 2. memory
  auto kill_workspace = [&](Workspace& w) {
    DeviceBuf* bufs[] = {&w.digits, &w.coarse_cnt, &w.region_start, &w.tmp_idx, &w.tmp_fine, &w.tmp_idx2, &w.tmp_fine2,
                         &w.mid_cnt, &w.region_start2, &w.bsize, &w.bstart, &w.istart, &w.win_items, &w.size_bins,
                         &w.sorted, &w.order, &w.multi_list, &w.redo_list, &w.counters, &w.bases29, &w.buckets, &w.item_partials,
                         &w.S, &w.T, &w.partial, &w.conv_scalars, &w.conv_points, &w.conv_tmp};
    for (DeviceBuf* b : bufs) kill_buf(*b);
  };
  auto kill_slot_memory = [](InstanceSlot& s) {
    if (s.h_partial) (void)hipHostFree(s.h_partial);
    s.h_partial = nullptr;
    s.h_partial_cap = 0;
  };
  for (Workspace& w : ctx->ws) kill_workspace(w);
  kill_workspace(ctx->g2.ws);
  for (DeviceBuf* b : {&ctx->g2.in_scalars, &ctx->g2.in_points}) kill_buf(*b);
  kill_slot_memory(ctx->g2.slot);
  for (CallState* cs : {&ctx->calls, &ctx->g2.calls}) cs->release(kill_buf, kill_event);
  handle_release_all(ctx->live_tables);   // handles the caller did not free
  handle_release_all(ctx->live_g2_tables);
  handle_release_all(ctx->live_ntt);
  handle_release_all(ctx->live_fr_mat);
  handle_release_all(ctx->live_poseidon);
  for (DeviceBuf* b : {&ctx->scratch_a, &ctx->scratch_b, &ctx->scratch_c, &ctx->scratch_b2, &ctx->scratch_c2}) kill_buf(*b);
  bases_cache_clear(ctx);   // (entries and unused reserves go through the graveyard)
  for (const msm_amd_ctx::CacheReserve& r : ctx->cache_reserve) ctx->graveyard.push_back(r.d);
  ctx->cache_reserve.clear();
  for (void* p : ctx->graveyard) (void)hipFree(p);
  ctx->graveyard.clear();
  for (Batch& B : ctx->batches) {
    for (InstanceSlot& s : B.slots) kill_slot_memory(s);
    B.slots.clear();
    B.active = B.abandoned = false;
  }
  for (auto& r : ctx->host_regs) (void)hipHostUnregister(const_cast<void*>(r.first));   // left registered by the caller
  ctx->host_regs.clear();
  (void)hipGetLastError();
  // 3. streams
  kill_stream(ctx->stream);
  for (hipStream_t& rs : ctx->reduce_streams) kill_stream(rs);
  kill_stream(ctx->front_stream);
  kill_stream(ctx->copy_stream);
  (void)hipGetLastError();
  lk.unlock();
  delete ctx;
}

// Page-locks a caller buffer for the life of the registration, so that the host-buffer entry points upload it by
// DMA at PCIe rate and without blocking the calling thread (pageable memory is staged by the runtime at roughly
// half that rate, on the calling thread).  Meant for long-lived inputs -- the bases of an SRS -- exactly the data
// the reference re-uploads on every call (msm.rs:152-153).  The caller keeps the memory valid and in place until
// msm_amd_host_unregister (or msm_amd_destroy).
int msm_amd_host_register(msm_amd_ctx* ctx, const void* ptr, size_t bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (!ptr || bytes == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer or empty range");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& r : ctx->host_regs)
    if (r.first == ptr) return fail(ctx, MSM_AMD_INPUT_ERROR, "range already registered");
  HIP_TRY(ctx, hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault));
  ctx->host_regs.emplace_back(ptr, bytes);
  return MSM_AMD_OK;
}

int msm_amd_host_unregister(msm_amd_ctx* ctx, const void* ptr) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (size_t i = 0; i < ctx->host_regs.size(); ++i)
    if (ctx->host_regs[i].first == ptr) {
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      if (!drain_or_mark_stalled(ctx))   // DMA from this buffer may still be in flight
        return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound: the buffer stays registered");
      HIP_TRY(ctx, hipHostUnregister(const_cast<void*>(ptr)));
      ctx->host_regs.erase(ctx->host_regs.begin() + (long)i);
      return MSM_AMD_OK;
    }
  return fail(ctx, MSM_AMD_INPUT_ERROR, "range was not registered on this ctx");
}

int msm_amd_set_window_size(msm_amd_ctx* ctx, uint32_t window_size) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (window_size != 0 && (window_size < kMinWindow || window_size > kMaxWindow))
    return fail(ctx, MSM_AMD_INPUT_ERROR, "window_size must be 0 (auto) or 3..17");
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->forced_window = window_size;
  return MSM_AMD_OK;
}

uint32_t msm_amd_auto_window_size(size_t n) { return auto_window(n); }
uint32_t msm_amd_auto_window_size_lone(size_t n) { return auto_window_lone(n); }
uint32_t msm_amd_auto_window_size_bounded(size_t n, uint32_t bits, int lone) {
  return auto_window_bounded(n, std::max(1u, std::min(bits, kModulusBits)), lone != 0);
}

int msm_amd_msm_batch(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                      const void* const* scalars, const void* const* points, const size_t* n, void* out) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  ++ctx->bases_cache_call;
  return run_batch_host(ctx, scalar_layout, point_layout, n_inst, scalars, points, n, out);
}

int msm_amd_set_bases_cache(msm_amd_ctx* ctx, size_t max_bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_streams_bounded(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy: bases cache left as it was");
  ctx->bases_cache_budget = max_bytes;
  ++ctx->bases_cache_call;
  while (ctx->bases_cache_bytes > max_bytes && !ctx->bases_cache.empty()) {   // least recently used first
    size_t victim = 0;
    for (size_t k = 1; k < ctx->bases_cache.size(); ++k)
      if (ctx->bases_cache[k].last_use < ctx->bases_cache[victim].last_use) victim = k;
    bases_cache_drop(ctx, victim);
  }
  return MSM_AMD_OK;
}

int msm_amd_set_bases_cache_verify(msm_amd_ctx* ctx, int full) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->bases_cache_verify = full ? 1 : 0;
  return MSM_AMD_OK;
}

// The caller's word that the array at host_points changed (or NULL: everything): its entries are dropped.
int msm_amd_bases_cache_invalidate(msm_amd_ctx* ctx, const void* host_points) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  for (size_t k = ctx->bases_cache.size(); k-- > 0;)
    if (!host_points || ctx->bases_cache[k].host == host_points) {
      ++ctx->bases_cache_invalidations;
      bases_cache_drop(ctx, k);   // the device copy goes to the graveyard: safe under work in flight
    }
  return MSM_AMD_OK;
}

int msm_amd_bases_cache_stats(msm_amd_ctx* ctx, uint64_t out[5]) {
  if (!ctx || !out) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  out[0] = ctx->bases_cache_hits;
  out[1] = ctx->bases_cache_misses;
  out[2] = ctx->bases_cache_invalidations;
  out[3] = ctx->bases_cache_bytes;
  out[4] = ctx->bases_cache.size();
  return MSM_AMD_OK;
}

int msm_amd_msm(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* scalars, const void* points,
                size_t n, void* out96) {
  return msm_amd_msm_batch(ctx, scalar_layout, point_layout, 1, &scalars, &points, &n, out96);
}

int msm_amd_gpu_msm_h2c(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, void* out96) {
  return msm_amd_msm(ctx, MSM_AMD_SCALAR_MONT_LE, MSM_AMD_POINT_H2C_AFFINE, scalars, points, n, out96);
}

int msm_amd_gpu_msm_h2c_sync(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n,
                             msm_amd_after_sort_fn after_sort, void* user, void* out96) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  if (!scalars || !points || !out96 || n == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "n == 0 or null pointer");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, ctx->scratch_b, n * 32))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, n * 64))) return rc;
  if ((rc = recover_if_stalled(ctx))) return rc;
  if ((rc = stage_upload(ctx, ctx->scratch_b.p, scalars, n * 32))) return rc;
  if ((rc = stage_upload(ctx, ctx->scratch_c.p, points, n * 64))) return rc;
  const void* ds = ctx->scratch_b.p;
  const void* dp = ctx->scratch_c.p;
  int ticket = -1;
  rc = submit_batch_device(ctx, MSM_AMD_SCALAR_MONT_LE, MSM_AMD_POINT_H2C_AFFINE, 1, &ds, &dp, &n, out96, &ticket);
  ctx->upload_pending = false;
  if (rc) return rc;
  ctx->after_sort_state = -1.0f;
  if (after_sort) {
    InstanceSlot& s = ctx->batches[ticket].slots[0];
    const hipError_t e = wait_event(s.ev[EV_SORT], ctx->wait_timeout_ms);   // sorted indices of this MSM exist (msm.rs:306-312)
    if (e == hipErrorNotReady) {
      ctx->stalled = true;
      ctx->batches[ticket].abandoned = true;
      return fail(ctx, MSM_AMD_PIPELINE_ERROR,
                  "timed out after " + std::to_string(ctx->wait_timeout_ms) + " ms waiting for event 'sort' of the MSM");
    }
    if (e != hipSuccess) {
      if (!drain_or_mark_stalled(ctx)) ctx->batches[ticket].abandoned = true;
      else ctx->batches[ticket].active = false;
      return fail(ctx, MSM_AMD_PIPELINE_ERROR, std::string("hipEventSynchronize(sort): ") + hipGetErrorString(e));
    }
    // a GPU-clock mark of "now" on a stream that has nothing queued: after the MSM has finished, the device time
    // from this mark to the end of bucket accumulation tells whether the callback ran while the GPU was still
    // accumulating (positive) -- host-side event queries race with the runtime's own polling
    if (!ctx->after_sort_mark) HIP_TRY(ctx, hipEventCreate(&ctx->after_sort_mark));
    HIP_TRY(ctx, hipEventRecord(ctx->after_sort_mark, ctx->copy_stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->after_sort_mark));   // the runtime submits lazily: make the mark real now
    after_sort(user);
    if (wait_event(s.ev[EV_ACC], ctx->wait_timeout_ms) == hipErrorNotReady) {
      ctx->stalled = true;
      ctx->batches[ticket].abandoned = true;
      return fail(ctx, MSM_AMD_PIPELINE_ERROR, "timed out after " + std::to_string(ctx->wait_timeout_ms) +
                                                   " ms waiting for event 'accumulate' of the MSM");
    }
    float lead = 0.0f;
    if (hipEventElapsedTime(&lead, ctx->after_sort_mark, s.ev[EV_ACC]) != hipSuccess) {
      (void)hipGetLastError();
      lead = 0.0f;
    }
    ctx->after_sort_state = lead > 0.0f ? 1.0f : 0.0f;
    ctx->after_sort_lead_ms = lead;
  }
  rc = wait_batch(ctx, ticket);
  ctx->after_sort_state = -1.0f;
  ctx->after_sort_lead_ms = 0.0f;
  return rc;
}

int msm_amd_metal_msm_ark(msm_amd_ctx* ctx, const void* points, const void* scalars, size_t n, void* out96) {
  return msm_amd_msm(ctx, MSM_AMD_SCALAR_MONT_LE, MSM_AMD_POINT_ARK_PROJECTIVE, scalars, points, n, out96);
}

// ---- hybrid front-end (src/metal/msm.rs:366-507) ---------------------------------------------------------
static size_t cpu_dispatch_below_fwd();
size_t msm_amd_reference_split(size_t n) {
  // gpu_with_cpu's split_at (msm.rs:377-383): the GPU gets the first n/3, n/2 or 2n/3 points
  if (n < ((size_t)1 << 18)) return n / 3;
  if (n < ((size_t)1 << 20)) return n / 2;
  return n * 2 / 3;
}

// The split measured on MI355X (tools/crossover.py, profiles/r03_crossover.txt): one GPU runs 2^20 points from host
// slices in ~3 ms, the host cores of a 16-thread grant need that long for ~2^14 points, so any share given to the CPU
// beyond msm_best's tiny-instance dispatch makes the call slower: everything goes to the GPU.
size_t msm_amd_tuned_split(size_t n) { return n < cpu_dispatch_below_fwd() ? 0 : n; }

int msm_amd_gpu_with_cpu(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, size_t split_at,
                         int cpu_threads, void* out96) {
  if (!ctx || !scalars || !points || !out96 || n == 0 || split_at > n)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad gpu_with_cpu arguments");
  if (cpu_threads <= 0) cpu_threads = msm_amd_host_threads();
  const u256* sc = (const u256*)scalars;
  const Affine* pt = (const Affine*)points;
  // CPU share on host threads (the reference waits for the GPU sort first because its sort borrows the CPU,
  // msm.rs:403-415; here the host cores are free from the start)
  Jacobian cpu_res = jac_identity();
  std::thread cpu_thread;
  const size_t n_cpu = n - split_at;
  bool cpu_ok = true;
  if (n_cpu) cpu_thread = std::thread([&] { cpu_res = host_msm(sc + split_at, 1, pt + split_at, n_cpu, cpu_threads, &cpu_ok); });
  Jacobian gpu_res = jac_identity();
  int rc = MSM_AMD_OK;
  if (split_at) {
    uint8_t buf[96];
    rc = msm_amd_msm(ctx, MSM_AMD_SCALAR_MONT_LE, MSM_AMD_POINT_H2C_AFFINE, scalars, points, split_at, buf);
    if (rc == MSM_AMD_OK) std::memcpy(&gpu_res, buf, 96);
  }
  if (n_cpu) cpu_thread.join();
  if (rc) return rc;
  if (!cpu_ok) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "gpu_with_cpu: host allocation failed in the CPU half");
  const Jacobian sum = normalise(jac_add(gpu_res, cpu_res));   // msm.rs:418-419
  std::memcpy(out96, &sum, 96);
  return MSM_AMD_OK;
}

// msm_best's size dispatch (msm.rs:440-444: `if n < 2^17 { cpu } else { gpu }`), threshold measured on MI355X with
// tools/crossover.py (profiles/r03_crossover.txt; round 2: r02_crossover.txt, 5 points): one blocking GPU call costs
// 0.28-0.38 ms of launches, event waits and host Horner whatever n is; the single-threaded host bucket method is faster
// than that up to 16 points (0.34 against 0.38 ms).
static size_t cpu_dispatch_below() {
  static const size_t v = [] {
    if (const char* e = std::getenv("MSM_AMD_CPU_BELOW")) return (size_t)std::strtoull(e, nullptr, 10);
    return (size_t)kCpuDispatchBelow;
  }();
  return v;
}

static size_t cpu_dispatch_below_fwd() { return cpu_dispatch_below(); }
size_t msm_amd_cpu_dispatch_below(void) { return cpu_dispatch_below(); }

int msm_amd_msm_best(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, void* out96) {
  if (!ctx || !scalars || !points || !out96 || n == 0 || n > 0x7FFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad msm_best arguments");
  if (n < cpu_dispatch_below()) {   // explicit size dispatch as in the reference, on a ctx that owns a GPU
    bool ok = true;
    const Jacobian r = normalise(host_msm((const u256*)scalars, 1, (const Affine*)points, n, 1, &ok));
    if (!ok) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "msm_best: host allocation failed");
    std::memcpy(out96, &r, 96);
    return MSM_AMD_OK;
  }
  std::unique_lock<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = recover_if_stalled(ctx))) return rc;
  const uint32_t nblocks = (uint32_t)((n + 1023) / 1024);
  if ((rc = ensure(ctx, ctx->scratch_b, n * 32))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, n * 64))) return rc;
  // filter_zeros (msm.rs:448-507): count the zero scalars on the device as soon as the scalars have arrived (the
  // points upload runs behind it), compact only if >= 30 % were zero (msm.rs:470)
  if ((rc = ensure(ctx, ctx->scratch_a, (((size_t)nblocks + 1) * 4 + 63) / 64 * 64 + n * 96))) return rc;
  uint32_t* counts = (uint32_t*)ctx->scratch_a.p;
  u256* f_sc = (u256*)((uint8_t*)ctx->scratch_a.p + (((size_t)nblocks + 1) * 4 + 63) / 64 * 64);
  Affine* f_pt = (Affine*)(f_sc + n);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_b.p, scalars, n * 32, hipMemcpyHostToDevice, st));
  launch_filter_count(st, (const u256*)ctx->scratch_b.p, (uint32_t)n, counts);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t survivors = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&survivors, counts + nblocks, 4, hipMemcpyDeviceToHost, st));
  // bases cache (opt-in, msm_amd_set_bases_cache): the converted resident copy stands in for upload + conversion; the
  // compaction below moves 64-byte records whatever their content, so it works on the converted form as well
  ++ctx->bases_cache_call;
  const void* dp = ctx->scratch_c.p;
  int pt_layout = MSM_AMD_POINT_H2C_AFFINE;
  BasesCacheEntry* hit = nullptr;
  AffPacked* fill = nullptr;
  if (ctx->bases_cache_budget) {
    bases_cache_reserve(ctx, 1, &points, &n, MSM_AMD_POINT_H2C_AFFINE);
    if ((hit = bases_cache_lookup(ctx, points, n, MSM_AMD_POINT_H2C_AFFINE)) == nullptr)
      if (BasesCacheEntry* f = bases_cache_insert(ctx, points, n, MSM_AMD_POINT_H2C_AFFINE)) fill = (AffPacked*)f->d_prepared;
  }
  if (hit) {
    dp = hit->d_prepared;
    pt_layout = MSM_AMD_POINT_PREPARED;
  } else {
    // an entry that was inserted for this call but never (provably) written must not be hit later: on any failure
    // from here to the end of the fill its key is cleared
    auto unkey = [&]() {
      if (fill)
        for (BasesCacheEntry& c : ctx->bases_cache)
          if (c.d_prepared == (void*)fill) c.host = nullptr;
    };
    hipError_t he = hipMemcpyAsync(ctx->scratch_c.p, points, n * 64, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && fill) {
      launch_convert_bases(st, (const Affine*)ctx->scratch_c.p, (uint32_t)n, fill);
      he = hipGetLastError();
      dp = fill;
      pt_layout = MSM_AMD_POINT_PREPARED;
    }
    if (he == hipSuccess) {
      if (int src_ = sync_stream_bounded(ctx, st, "msm_best upload")) {
        unkey();
        return src_;
      }
    }
    if (he != hipSuccess) {
      unkey();
      HIP_TRY(ctx, he);
    }
  }
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  const double zero_ratio = (double)(n - survivors) / (double)n;
  const void* ds = ctx->scratch_b.p;
  size_t m = n;
  if (zero_ratio >= 0.30) {   // msm.rs:470
    launch_filter_scatter(st, (const u256*)ctx->scratch_b.p, (const Affine*)dp, (uint32_t)n, counts, f_sc, f_pt);
    HIP_TRY(ctx, hipGetLastError());
    if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;   // run_batch_device starts on the front stream
    ds = f_sc;
    dp = f_pt;
    m = survivors;
  }
  if (m == 0) {   // every scalar is zero: the sum is the identity
    const Jacobian id = jac_identity();
    std::memcpy(out96, &id, 96);
    return MSM_AMD_OK;
  }
  return run_batch_device(ctx, MSM_AMD_SCALAR_MONT_LE, pt_layout, 1, &ds, &dp, &m, out96);
}

int msm_amd_msm_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                             const void* const* d_scalars, const void* const* d_points, const size_t* n,
                             void* out_host) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return run_batch_device(ctx, scalar_layout, point_layout, n_inst, d_scalars, d_points, n, out_host);
}

int msm_amd_submit_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                void* out_host, int* ticket) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return submit_batch_device(ctx, scalar_layout, point_layout, n_inst, d_scalars, d_points, n, out_host, ticket);
}

int msm_amd_wait_batch(msm_amd_ctx* ctx, int ticket) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return wait_batch(ctx, ticket, false);
}

int msm_amd_set_wait_timeout_ms(msm_amd_ctx* ctx, uint32_t timeout_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->wait_timeout_ms = timeout_ms;
  return MSM_AMD_OK;
}

int msm_amd_msm_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* d_scalars,
                       const void* d_points, size_t n, void* out96_host) {
  return msm_amd_msm_batch_device(ctx, scalar_layout, point_layout, 1, &d_scalars, &d_points, &n, out96_host);
}

// ---- scalars of bounded width: the entry points above with a plan of bits / c + 1 windows (make_plan) ------------------
int msm_amd_msm_bounded(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* scalars, const void* points,
                        size_t n, uint32_t bits, int sign, void* out96) {
  if (int rc = bound_args(ctx, __func__, bits, sign)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  ++ctx->bases_cache_call;
  BoundScope scope(ctx, bits, sign);
  return run_batch_host(ctx, scalar_layout, point_layout, 1, &scalars, &points, &n, out96);
}

int msm_amd_msm_batch_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                     const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                     uint32_t bits, int sign, void* out_host) {
  if (int rc = bound_args(ctx, __func__, bits, sign)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  BoundScope scope(ctx, bits, sign);
  return run_batch_device(ctx, scalar_layout, point_layout, n_inst, d_scalars, d_points, n, out_host);
}

int msm_amd_submit_batch_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                        const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                        uint32_t bits, int sign, void* out_host, int* ticket) {
  if (int rc = bound_args(ctx, __func__, bits, sign)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  BoundScope scope(ctx, bits, sign);
  return submit_batch_device(ctx, scalar_layout, point_layout, n_inst, d_scalars, d_points, n, out_host, ticket);
}

int msm_amd_msm_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* d_scalars,
                               const void* d_points, size_t n, uint32_t bits, int sign, void* out96_host) {
  return msm_amd_msm_batch_bounded_device(ctx, scalar_layout, point_layout, 1, &d_scalars, &d_points, &n, bits, sign,
                                          out96_host);
}

// Conversion of a resident point array to the internal packed form; ctx->mu held by the caller.
static int prepare_bases_locked(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, void* d_prepared) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");   // a set-up step: the conversion scratch of workspace 0 must be idle
  hipStream_t st = ctx->stream;
  const Affine* pts = nullptr;
  if (int rc = convert_points(ctx, ctx->ws[0], st, point_layout, d_points, n, &pts)) return rc;
  launch_convert_bases(st, pts, (uint32_t)n, (AffPacked*)d_prepared);
  HIP_TRY(ctx, hipGetLastError());
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_bases_prepare_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, void* d_prepared) {
  if (!ctx || !d_points || !d_prepared || n == 0 || n > 0xFFFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad bases_prepare arguments");
  if (point_layout == MSM_AMD_POINT_PREPARED || point_bytes(point_layout) == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad point layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  return prepare_bases_locked(ctx, point_layout, d_points, n, d_prepared);
}

int msm_amd_bases_upload(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, void** d_prepared) {
  if (!ctx || !points || !d_prepared || n == 0 || n > 0xFFFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad bases_upload arguments");
  const size_t pb = point_bytes(point_layout);
  if (pb == 0 || point_layout == MSM_AMD_POINT_PREPARED) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad point layout");
  *d_prepared = nullptr;
  std::lock_guard<std::mutex> g(ctx->mu);
  return upload_and_prepare(
      ctx, ctx->scratch_c, points, n * pb, n * sizeof(AffPacked), "the resident copy of the bases",
      [&](const void* staged, void* d_out) { return prepare_bases_locked(ctx, point_layout, staged, n, d_out); },
      d_prepared);
}

// ---- precomputed window tables ------------------------------------------------------------
static uint32_t auto_table_window(size_t n) {
  // One bucket set serves all windows, so the window can grow until the 2^(c-1) buckets of the window reduction
  // (2 full additions each) cost as much as the mixed additions they save.  Windows whose top digit is narrow are
  // excluded: the n entries of the top window would all fall into its few slots (c = 19 leaves 7 bits for the top
  // window of a 254-bit scalar: 2^20 entries in 128 buckets and in ONE region of the sort).
  uint32_t best = 4;
  double best_cost = 1e300;
  for (uint32_t c = 4; c <= 21; ++c) {
    const uint32_t W = kModulusBits / c + 1;
    const uint32_t top = kModulusBits - (W - 1) * c;          // bits of the top window
    if (top + 6 < c && c > 6) continue;                        // top window concentrated > 64-fold
    if ((size_t)W * n > 0x7FFFFFFFull) continue;
    const double cost = 9.5 * (double)W * (double)n + 27.0 * (double)((size_t)1 << (c - 1)) + 14.0 * (double)W * (double)n / 32.0;
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

static int tables_build_locked(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, uint32_t window_size,
                               msm_amd_tables** out) {
  uint32_t c, W;
  if (int grc = tables_geometry(ctx, n, window_size, auto_table_window(n), &c, &W)) return grc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_or_mark_stalled(ctx)) return fail(ctx, MSM_AMD_PIPELINE_ERROR, "device busy past the wait bound");   // a set-up step: the conversion scratch of workspace 0 must be idle
  hipStream_t st = ctx->stream;
  const Affine* pts = nullptr;
  if (point_layout == MSM_AMD_POINT_PREPARED || point_layout == MSM_AMD_POINT_TABLES)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "tables are built from one of the host point layouts");
  if (int rc = convert_points(ctx, ctx->ws[0], st, point_layout, d_points, n, &pts)) return rc;
  return tables_build_tail(ctx, ctx->live_tables, n, c, W, sizeof(AffPacked), "",
                           [&](void* d_tab) { launch_build_tables(st, pts, (uint32_t)n, c, W, (AffPacked*)d_tab); }, out);
}

int msm_amd_tables_build_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, uint32_t window_size,
                                msm_amd_tables** out) {
  if (!ctx || !d_points || !out || n == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad tables_build arguments");
  *out = nullptr;
  if (point_bytes(point_layout) == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown point layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  return tables_build_locked(ctx, point_layout, d_points, n, window_size, out);
}

int msm_amd_tables_build(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, uint32_t window_size,
                         msm_amd_tables** out) {
  if (!ctx || !points || !out || n == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad tables_build arguments");
  *out = nullptr;
  const size_t pb = point_bytes(point_layout);
  if (pb == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown point layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, ctx->scratch_c, n * pb))) return rc;
  HIP_TRY(ctx, hipMemcpy(ctx->scratch_c.p, points, n * pb, hipMemcpyHostToDevice));
  return tables_build_locked(ctx, point_layout, ctx->scratch_c.p, n, window_size, out);
}

int msm_amd_tables_info(msm_amd_ctx* ctx, const msm_amd_tables* tables, size_t* n, uint32_t* window_size,
                        uint32_t* num_windows, size_t* device_bytes) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return tables_info(ctx, ctx->live_tables, tables, "not a table handle of this ctx", n, window_size,
                     num_windows, device_bytes);
}

int msm_amd_tables_free(msm_amd_ctx* ctx, msm_amd_tables* tables) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  return handle_free(ctx, ctx->live_tables, tables, "not a table handle of this ctx");
}

int msm_amd_msm_tables(msm_amd_ctx* ctx, const msm_amd_tables* tables, int scalar_layout, const void* scalars,
                       void* out96) {
  if (!ctx || !tables || !scalars || !out96) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad msm_tables arguments");
  if (!scalar_layout_ok(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  const msm_amd_tables* t = find_handle(ctx->live_tables, tables);
  if (!t) return fail(ctx, MSM_AMD_INPUT_ERROR, "not a table handle of this ctx");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  const size_t n = t->n;
  if ((rc = recover_if_stalled(ctx))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, n * 32))) return rc;
  if ((rc = stage_upload(ctx, ctx->scratch_b.p, scalars, n * 32))) return rc;
  const void* ds = ctx->scratch_b.p;
  const void* dp = tables;
  rc = run_batch_device(ctx, scalar_layout, MSM_AMD_POINT_TABLES, 1, &ds, &dp, &n, out96);
  ctx->upload_pending = false;
  return rc;
}

int msm_amd_msm_prepared(msm_amd_ctx* ctx, int scalar_layout, const void* scalars, const void* d_prepared, size_t n,
                         void* out96) {
  if (!ctx || !scalars || !d_prepared || !out96 || n == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad msm_prepared arguments");
  if (!scalar_layout_ok(scalar_layout)) return fail(ctx, MSM_AMD_INPUT_ERROR, "unknown scalar layout");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = recover_if_stalled(ctx))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, n * 32))) return rc;
  if ((rc = stage_upload(ctx, ctx->scratch_b.p, scalars, n * 32))) return rc;
  const void* ds = ctx->scratch_b.p;
  rc = run_batch_device(ctx, scalar_layout, MSM_AMD_POINT_PREPARED, 1, &ds, &d_prepared, &n, out96);
  ctx->upload_pending = false;
  return rc;
}

int msm_amd_device_alloc(msm_amd_ctx* ctx, size_t bytes, void** d_ptr) {
  if (!ctx || !d_ptr || bytes == 0) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad device_alloc arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = quiesce_for_allocation(ctx, "device memory (msm_amd_device_alloc)")) return rc;
  HIP_TRY(ctx, hipMalloc(d_ptr, bytes));
  return MSM_AMD_OK;
}

int msm_amd_device_free(msm_amd_ctx* ctx, void* d_ptr) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!d_ptr) return MSM_AMD_OK;
  if (!drain_streams_bounded(ctx)) {   // the device does not answer: hipFree would wait for it without bound
    ctx->graveyard.push_back(d_ptr);   // released once the ctx is idle again, or at msm_amd_destroy
    return MSM_AMD_OK;
  }
  HIP_TRY(ctx, hipFree(d_ptr));
  return MSM_AMD_OK;
}

int msm_amd_copy_to_device(msm_amd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  if (!ctx || !d_dst || !h_src) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  if (int src_ = sync_stream_bounded(ctx, ctx->stream, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_copy_to_host(msm_amd_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
  if (!ctx || !h_dst || !d_src) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (int src_ = sync_stream_bounded(ctx, ctx->stream, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_ctx_device(const msm_amd_ctx* ctx) { return ctx ? ctx->device : -1; }

void* msm_amd_stream(msm_amd_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int msm_amd_synchronize(msm_amd_ctx* ctx) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!drain_streams_bounded(ctx)) {
    ctx->stalled = true;
    return fail(ctx, MSM_AMD_PIPELINE_ERROR,
                "timed out after " + std::to_string(ctx->wait_timeout_ms) + " ms waiting for the ctx's streams to drain");
  }
  HIP_TRY(ctx, hipGetLastError());
  return recover_if_stalled(ctx);
}

int msm_amd_generate_instance(msm_amd_ctx* ctx, uint64_t seed, size_t n, int scalars_mont, void* d_points,
                              void* d_scalars) {
  if (!ctx || !d_points || !d_scalars || n == 0 || n > 0x7FFFFFFFull)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad generate_instance arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_gen_instance(ctx->stream, seed, (uint32_t)n, scalars_mont, (Affine*)d_points, (u256*)d_scalars);
  HIP_TRY(ctx, hipGetLastError());
  if (int src_ = sync_stream_bounded(ctx, ctx->stream, __func__)) return src_;
  return MSM_AMD_OK;
}

// ---- per-stage entry points ------------------------------------------------------------------------
int msm_amd_prepare_buckets_indices(msm_amd_ctx* ctx, const uint32_t* scalars_be32, size_t n, uint32_t window_size,
                                    uint32_t num_windows, uint32_t* pairs_out) {
  if (!ctx || !scalars_be32 || !pairs_out || n == 0 || window_size == 0 || window_size > 32 || num_windows == 0)
    return fail(ctx, MSM_AMD_INPUT_ERROR, "bad prepare_buckets_indices arguments");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  const size_t pair_bytes = n * num_windows * 8;
  if ((rc = ensure(ctx, ctx->scratch_a, n * 32))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, n * 32))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, pair_bytes))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, scalars_be32, n * 32, hipMemcpyHostToDevice, st));
  launch_be32_to_le(st, (const uint32_t*)ctx->scratch_a.p, n, (uint32_t*)ctx->scratch_b.p);
  launch_ref_prepare(st, (const u256*)ctx->scratch_b.p, (uint32_t)n, window_size, num_windows,
                     (uint2*)ctx->scratch_c.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(pairs_out, ctx->scratch_c.p, pair_bytes, hipMemcpyDeviceToHost, st));
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_sort_buckets_indices(msm_amd_ctx* ctx, uint32_t* pairs, size_t n_pairs) {
  if (!ctx || !pairs) return fail(ctx, MSM_AMD_INPUT_ERROR, "null pointer");
  if (n_pairs == 0) return MSM_AMD_OK;
  if (n_pairs > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "too many pairs");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  const uint32_t tiles = (uint32_t)((n_pairs + kRadixTile - 1) / kRadixTile);
  if ((rc = ensure(ctx, ctx->scratch_a, n_pairs * 8))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, n_pairs * 8))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, ((size_t)tiles + 1) * 256 * 4))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, pairs, n_pairs * 8, hipMemcpyHostToDevice, st));
  uint2* src = nullptr;
  launch_radix_sort_pairs(st, (uint2*)ctx->scratch_a.p, (uint2*)ctx->scratch_b.p, n_pairs,
                          (uint32_t*)ctx->scratch_c.p, &src);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(pairs, src, n_pairs * 8, hipMemcpyDeviceToHost, st));
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
  return MSM_AMD_OK;
}

int msm_amd_sort_pairs_device(msm_amd_ctx* ctx, void* d_pairs, size_t n_pairs, uint32_t key_bits, float* kernel_ms) {
  if (!ctx || !d_pairs || key_bits == 0 || key_bits > 32) return fail(ctx, MSM_AMD_INPUT_ERROR, "bad sort arguments");
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_pairs == 0) return MSM_AMD_OK;
  if (n_pairs > 0xFFFFFFFFull) return fail(ctx, MSM_AMD_INPUT_ERROR, "too many pairs");
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  const uint32_t tiles = (uint32_t)((n_pairs + kRadixTile - 1) / kRadixTile);
  if ((rc = ensure(ctx, ctx->scratch_b, n_pairs * 8))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, ((size_t)tiles + 1) * 256 * 4))) return rc;
  hipEvent_t e0, e1;
  HIP_TRY(ctx, hipEventCreate(&e0));
  HIP_TRY(ctx, hipEventCreate(&e1));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  uint2* src = nullptr;
  launch_radix_sort_pairs(st, (uint2*)d_pairs, (uint2*)ctx->scratch_b.p, n_pairs, (uint32_t*)ctx->scratch_c.p, &src,
                          key_bits);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess && src != (uint2*)d_pairs)   // odd number of passes: the result sits in the scratch buffer
    le = hipMemcpyAsync(d_pairs, src, n_pairs * 8, hipMemcpyDeviceToDevice, st);
  if (le == hipSuccess) le = hipEventRecord(e1, st);
  if (le == hipSuccess && sync_stream_bounded(ctx, st, "pair sort")) le = hipErrorNotReady;
  float ms = 0.f;
  if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIP_TRY(ctx, le);
  if (kernel_ms) *kernel_ms = ms;
  return MSM_AMD_OK;
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

size_t msm_amd_scalar_bytes(int scalar_layout) {
  return (scalar_layout == MSM_AMD_SCALAR_MONT_LE || scalar_layout == MSM_AMD_SCALAR_CANON_LE ||
          scalar_layout == MSM_AMD_SCALAR_CANON_BE32) ? 32 : 0;
}
size_t msm_amd_point_bytes(int point_layout) { return point_bytes(point_layout); }

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
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  size_t wa, wb;
  test_op_widths(op, &wa, &wb);
  const size_t wo = wa;
  std::vector<uint32_t> la(count * wa * 8), lb(count * wb * 8), lo(count * wo * 8);
  for (size_t i = 0; i < count * wa; ++i)
    for (int l = 0; l < 8; ++l) la[i * 8 + l] = a[i * 8 + 7 - l];
  for (size_t i = 0; i < count * wb; ++i)
    for (int l = 0; l < 8; ++l) lb[i * 8 + l] = b[i * 8 + 7 - l];
  int rc;
  if ((rc = ensure(ctx, ctx->scratch_a, la.size() * 4))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, lb.size() * 4))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, lo.size() * 4))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, la.data(), la.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_b.p, lb.data(), lb.size() * 4, hipMemcpyHostToDevice, st));
  launch_test_op(st, op, (const u256*)ctx->scratch_a.p, (const u256*)ctx->scratch_b.p, (u256*)ctx->scratch_c.p,
                 (uint32_t)count);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(lo.data(), ctx->scratch_c.p, lo.size() * 4, hipMemcpyDeviceToHost, st));
  if (int src_ = sync_stream_bounded(ctx, st, __func__)) return src_;
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
  std::lock_guard<std::mutex> g(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t in_bytes = count * kRawInWords * 4, out_bytes = count * kRawOutWords * 4;
  int rc;
  if ((rc = ensure(ctx, ctx->scratch_a, in_bytes))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, in_bytes))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, out_bytes))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, a, in_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_b.p, b, in_bytes, hipMemcpyHostToDevice, st));
  if (op == MSM_AMD_RAW_FE_SQRT)   // the root ladder has a kernel of its own (k_compress.hip)
    launch_sqrt_raw(st, false, (const uint32_t*)ctx->scratch_a.p, (uint32_t*)ctx->scratch_c.p, (uint32_t)count);
  else
    launch_test_op_raw(st, op, (const uint32_t*)ctx->scratch_a.p, (const uint32_t*)ctx->scratch_b.p,
                       (uint32_t*)ctx->scratch_c.p, (uint32_t)count);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->scratch_c.p, out_bytes, hipMemcpyDeviceToHost, st));
  return sync_stream_bounded(ctx, st, __func__);
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

int msm_amd_last_timings(const msm_amd_ctx* ctx, msm_amd_timings* out) {
  if (!ctx || !out) return MSM_AMD_INPUT_ERROR;
  *out = ctx->timings;
  return MSM_AMD_OK;
}

uint64_t msm_amd_algorithmic_bytes(size_t n, uint32_t window_size, int accumulate_only) {
  // A(n) = 32n + 72nW + 2*96*totB ; A3(n) = 72nW + 96*totB, with
  // totB = W * (2^c - 1), 64-byte affine bases, 8-byte (bucket, point) pairs, 96-byte buckets.
  const uint64_t c = window_size ? window_size : auto_window(n);
  const uint64_t W = (kModulusBits + c - 1) / c;
  const uint64_t totB = W * ((1ull << c) - 1);
  if (accumulate_only) return 72ull * n * W + 96ull * totB;
  return 32ull * n + 72ull * n * W + 2ull * 96ull * totB;
}

}  // extern "C"

// ---- BN254 G2 MSM (one blocking call on the main stream) -----------------------------------------------------------
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
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t in_bytes = count * kG2RawIn * 4, out_bytes = count * kG2RawOut * 4;
  int rc;
  if ((rc = ensure(ctx, ctx->scratch_a, in_bytes))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_b, in_bytes))) return rc;
  if ((rc = ensure(ctx, ctx->scratch_c, out_bytes))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_a.p, a, in_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scratch_b.p, b, in_bytes, hipMemcpyHostToDevice, st));
  if (op == MSM_AMD_G2_RAW_FQ2_SQRT)
    launch_sqrt_raw(st, true, (const uint32_t*)ctx->scratch_a.p, (uint32_t*)ctx->scratch_c.p, (uint32_t)count);
  else
    launch_test_op_g2(st, op, (const uint32_t*)ctx->scratch_a.p, (const uint32_t*)ctx->scratch_b.p,
                      (uint32_t*)ctx->scratch_c.p, (uint32_t)count);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out, ctx->scratch_c.p, out_bytes, hipMemcpyDeviceToHost, st));
  return sync_stream_bounded(ctx, st, __func__);
}

}  // extern "C"

// ---- the blocking vector calls: the point calls of both groups, the transform, the vectors over Fr ------------------------
// One driver for all of them (device_call): the device set, a bounded drain of the ctx's earlier work, every buffer sized
// on the idle ctx before anything is enqueued, host input through the page-locked staging ring, the caller's kernels on
// the main stream (between events when the call is timed), the 64-byte record of a call that has one behind a bounded
// wait, output and reason bytes behind a bounded stream wait.  Each call below validates its own arguments, takes
// ctx->mu, describes its buffers in a DeviceCall and passes a callable that enqueues its kernels; one that takes the
// finished record, and the kernels that follow it, are optional.
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

int fr_prefix_call(msm_amd_ctx* ctx, bool host, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, void* out,
                   float* kernel_ms) {
  if (!ctx) return MSM_AMD_INPUT_ERROR;
  DeviceCall d;
  d.who = host ? "msm_amd_fr_prefix_product" : "msm_amd_fr_prefix_product_device";
  if (kernel_ms) *kernel_ms = 0.f;
  if (!fr_mode_known(mode))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": mode must be MSM_AMD_FR_PREFIX_INCLUSIVE or MSM_AMD_FR_PREFIX_EXCLUSIVE");
  if (const char* why = fr_unary_check(scalar_layout, in, n, n_vec, out, !host))
    return fail(ctx, MSM_AMD_INPUT_ERROR, d.who + ": " + why);
  if (n == 0 || n_vec == 0) return MSM_AMD_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CallState& s = ctx->calls;
  FrScanLaunch c{};
  c.n = n, c.n_vec = n_vec, c.tile_log = ctx->fr_tile_log, c.layout = scalar_layout, c.mode = mode;
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
  return fr_prefix_call(ctx, true, scalar_layout, mode, in, n, n_vec, out, nullptr);
}

int msm_amd_fr_prefix_product_device(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* d_in, size_t n, size_t n_vec,
                                     void* d_out, float* kernel_ms) {
  return fr_prefix_call(ctx, false, scalar_layout, mode, d_in, n, n_vec, d_out, kernel_ms);
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
// msm_amd_fr_sumcheck_round*) ------------------------------------------------------------------------------------------------
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

}  // namespace

extern "C" {

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
