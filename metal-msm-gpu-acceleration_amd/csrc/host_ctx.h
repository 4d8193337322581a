// The ctx of the host driver and what its translation units share: the constants and types of msm_host.hip (the MSM
// driver) that calls_points.hip, calls_ntt.hip and calls_fr.hip (the blocking vector calls, through device_call.h) see as
// well, HIP_TRY, the handle templates, and the declarations of the helpers those units call.  Private to csrc/: not
// installed.  The helpers are defined in msm_host.hip.  They, and the two types that msm_host.hip had in its anonymous
// namespace (every unit must see the same ones now), are in msm_amd::drv, with hidden visibility, so that nothing here
// becomes an exported name of the library (the attribute does not carry over to a reopened namespace: msm_host.hip
// repeats it).  The list is closed on purpose: nothing of the planner, the instance pipeline, the uploader or the bases
// cache is declared here; what the units of the MSM driver itself (msm_host.hip, msm_plan.hip, msm_g2.hip,
// calls_stages.hip) take from each other is in msm_driver.h, which the vector calls do not include.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/msm_amd.h"
#include "device_common.hip.h"
#include "launch.h"
#include "launch_check.h"
#include "launch_fr.h"
#include "launch_ntt.h"

using namespace msm_amd;

namespace msm_amd {
namespace drv __attribute__((visibility("hidden"))) {

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

}  // namespace drv
}  // namespace msm_amd

using namespace msm_amd::drv;

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

// A lookup table over Fr (msm_amd_fr_lookup_*, msm_amd_ctx::live_fr_lookup): d_mem is the image of fr_lookup_plan -- the
// rows as reduced Montgomery residues, the slots of the index, the statistics of the build.
struct msm_amd_fr_lookup : DeviceHandle {
  uint64_t n_rows = 0, n_distinct = 0, longest_probe = 0;
  FrLookupPlan plan{};
  bool sorted = false;   // msm_amd_fr_lookup_build_sorted: row k is sorted position k of the caller's table
};

// Buffers of the blocking vector calls (device_call.h): the staging of the host-buffer forms, the 64-byte record a
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
  std::vector<msm_amd_fr_lookup*> live_fr_lookup;   // last: every member above keeps its place
};

namespace msm_amd {
namespace drv __attribute__((visibility("hidden"))) {

int fail(msm_amd_ctx* ctx, int status, const std::string& msg);
int recover_if_stalled(msm_amd_ctx* ctx);
int quiesce_for_allocation(msm_amd_ctx* ctx, const char* what);
int sync_stream_bounded(msm_amd_ctx* ctx, hipStream_t st, const char* what);
// Error paths and set-up steps: the bounded drain; a device that does not get there leaves the ctx marked stalled (the
// next entry point checks whether it has caught up) instead of holding the caller.
bool drain_or_mark_stalled(msm_amd_ctx* ctx);
int ensure(msm_amd_ctx* ctx, DeviceBuf& b, size_t bytes);
float event_span(hipEvent_t a, hipEvent_t b);
int staged_upload(msm_amd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t stream);

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

// ---- handles: H = msm_amd_tables (ctx->live_tables), msm_amd_g2_tables (ctx->live_g2_tables), msm_amd_ntt_domain
// (ctx->live_ntt), msm_amd_fr_matrix (ctx->live_fr_mat), msm_amd_poseidon_params (ctx->live_poseidon) or msm_amd_fr_lookup
// (ctx->live_fr_lookup).  ctx->mu is held by the caller, as for every helper here.
template <class H>
const H* find_handle(const std::vector<H*>& live, const void* handle) {
  for (const H* t : live)
    if ((const void*)t == handle) return t;
  return nullptr;
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

}  // namespace drv
}  // namespace msm_amd
