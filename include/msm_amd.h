/* msm_amd.h -- C ABI of the MI355X-native BN254 G1 multi-scalar multiplication (libmsm_amd.so).
 *
 * Drop-in boundary for the Apple-Metal MSM path of ElusAegis/metal-msm-gpu-acceleration (crate
 * `mopro-msm`).  The reference has no C ABI of its own (its callers are generic Rust functions,
 * src/metal/msm.rs); every entry point below cites the reference interface it replaces, and
 * INTEGRATION.md shows the Rust `extern "C"` shim a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types;
 *   - every function returns an int status (0 = OK), never aborts;
 *   - a ctx owns one HIP device, four HIP streams (front end, accumulate, two reduce streams: consecutive
 *     instances overlap their phases) plus a copy stream, and grow-on-demand device workspaces; calls on one ctx are
 *     serialised internally, different ctxs (one per GPU, or several on one GPU) run concurrently -- see
 *     msm_amd_msm_batch_multi;
 *   - all 256-bit values are little-endian (least significant byte first) unless a *_BE32 layout
 *     is named; field coordinates are in Montgomery form with R = 2^256 exactly as halo2curves and
 *     arkworks hold them in memory.
 */
#ifndef MSM_AMD_H
#define MSM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msm_amd_ctx msm_amd_ctx;

/* Status codes; 1..5 mirror MetalError (src/metal/abstraction/errors.rs:4-19). */
enum {
  MSM_AMD_OK = 0,
  MSM_AMD_DEVICE_NOT_FOUND = 1, /* MetalError::DeviceNotFound */
  MSM_AMD_LIBRARY_ERROR = 2,    /* MetalError::LibraryError   (code object missing / not gfx950) */
  MSM_AMD_FUNCTION_ERROR = 3,   /* MetalError::FunctionError  (kernel attribute / symbol) */
  MSM_AMD_PIPELINE_ERROR = 4,   /* MetalError::PipelineError  (launch / runtime failure) */
  MSM_AMD_INPUT_ERROR = 5,      /* MetalError::InputError     (null, n == 0, bad layout/size) */
  /* 6..8 mirror HarnessError of the instance-file harness (src/utils/preprocess.rs:11-21). */
  MSM_AMD_FILE_OPEN_ERROR = 6,        /* HarnessError::FileOpenError        (open/read/write failed) */
  MSM_AMD_DESERIALIZATION_ERROR = 7,  /* HarnessError::DeserializationError (truncated or malformed bincode) */
  MSM_AMD_INVALID_DATA = 8            /* HarnessError::InvalidData          (instance count / size mismatch) */
};

/* Scalar layouts (32 bytes each). */
enum {
  MSM_AMD_SCALAR_MONT_LE = 0,   /* halo2curves bn256::Fr / ark_bn254::Fr in memory: [u64;4] LE, Montgomery
                                   (msm.rs:258-270 reinterprets &[C::Scalar]) */
  MSM_AMD_SCALAR_CANON_LE = 1,  /* canonical integer, little-endian */
  MSM_AMD_SCALAR_CANON_BE32 = 2 /* reference wire layout: 8 x u32, most significant limb first, canonical
                                   (limbs_conversion.rs:116-121, :282-288) */
};

/* Point layouts. */
enum {
  MSM_AMD_POINT_H2C_AFFINE = 0,     /* bn256::G1Affine {x,y}: 64 B, Montgomery LE, identity = (0,0) */
  MSM_AMD_POINT_ARK_PROJECTIVE = 1, /* ark_bn254::G1Projective {x,y,z}: 96 B Jacobian, Montgomery LE
                                       (limbs_conversion.rs:123-130) */
  MSM_AMD_POINT_ARK_AFFINE = 2,     /* ark_bn254::G1Affine {x,y,infinity:bool}: 72 B (limbs_conversion.rs:132-137) */
  MSM_AMD_POINT_JAC_BE32 = 3,       /* reference wire layout: 24 x u32 (x,y,z each MS-limb first), Montgomery */
  MSM_AMD_POINT_PREPARED = 4,       /* device-only: 64-byte records written by msm_amd_bases_upload /
                                       msm_amd_bases_prepare_device (opaque internal form of affine points) */
  MSM_AMD_POINT_TABLES = 5          /* the "points" pointer is a msm_amd_tables handle (precomputed window tables) */
};

/* Per-stage device times of the last MSM on this ctx, milliseconds, from hipEvents on the ctx stream
 * (replaces the log::debug! Instant timers of msm.rs:193-214, 288-328).  A G1 instance and a G2 call run the same
 * instance body with the same stage events, so every field means the same for both groups. */
typedef struct msm_amd_timings {
  float convert_ms;     /* input layout conversion (0 when inputs are already native) */
  float digits_ms;      /* prepare_buckets_indices */
  float sort_ms;        /* sort_buckets: hist + prefix + scan + scatter (+ bucket ordering) */
  float accumulate_ms;  /* bucket_wise_accumulation (dominant kernel): the accumulate kernel alone */
  float reduce_ms;      /* the combine pass over split buckets, then sum_reduction (segment + tree kernels) and the copy
                           of its partial points */
  float final_ms;       /* final_accumulation on the host (wall clock) */
  float total_gpu_ms;   /* SUM of the stage spans above (stages of neighbouring instances overlap on other streams,
                           so this is not a wall interval) */
  uint32_t n;
  uint32_t window_size;
  uint32_t num_windows;
  uint32_t reserved;            /* number of instances the averages were taken over; for ONE large instance that ran
                                   as pipelined point ranges (lone calls from 2^23 device-resident / 2^19 host points,
                                   MSM_AMD_SPLIT): the number of ranges, and the stage fields are SUMS over them */
  float accumulate_kernel_ms;   /* accumulate_kernel alone (events directly around its launch) */
  float reserved2[3];           /* [0] = work items of the last instance's accumulate grid (exact below 2^24)
                                   [1] = 1 if bucket accumulation had not finished yet when the after_sort
                                         callback of msm_amd_gpu_msm_h2c_sync fired, 0 if it had, -1 if no callback ran
                                   [2] = device time (ms) from that callback to the end of bucket accumulation */
} msm_amd_timings;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* setup_metal_state (msm.rs:77-94): pick `device` (ordinal; -1 = current HIP device), create the
 * stream, check the kernels are loadable. */
int msm_amd_init(int device, msm_amd_ctx** out);
/* setup_metal_state_reusable (msm.rs:96-109): process-global cached ctx on the current device. */
int msm_amd_init_reusable(msm_amd_ctx** out);
/* get_global_metal_config (msm.rs:114-119): the cached ctx, MSM_AMD_INPUT_ERROR if never initialised. */
int msm_amd_get_global(msm_amd_ctx** out);
void msm_amd_destroy(msm_amd_ctx* ctx);
const char* msm_amd_strerror(int status);
/* Human-readable detail of the last failure on this ctx (empty string if none). */
const char* msm_amd_last_error(const msm_amd_ctx* ctx);

/* encode_instances' `window_size: Option<u32>` (msm.rs:130-141): 0 = automatic, else 3..17. */
int msm_amd_set_window_size(msm_amd_ctx* ctx, uint32_t window_size);
/* The automatic choice for n points.  Reference policy: 3 if n < 32 else 15 (msm.rs:135-141).  This library: 3 below
 * 32 points, then the window measured fastest on MI355X per size class (5 up to 2^14 points, 15 up
 * to 2^18, 16 at 2^19, 17 beyond) for instances that run PIPELINED (batches, or a call submitted while others are
 * in flight); results never depend on it. */
uint32_t msm_amd_auto_window_size(size_t n);
/* The automatic choice for ONE instance submitted while nothing else is in flight (a blocking gpu_msm_h2c call):
 * such a call is a chain of launches and dependent additions, not a throughput problem, and wider windows with a
 * full top digit are faster (5 up to 2^6 points, 8 up to 2^12, 15 up to 2^18, 17 beyond). */
uint32_t msm_amd_auto_window_size_lone(size_t n);

/* ---- whole-MSM entry points: host buffers ---------------------------------------------------- */
/* gpu_msm_h2c::<G1Affine, .., Fr>(scalars, points) -> G1 (msm.rs:352-364).
 * scalars: n x 32 B MSM_AMD_SCALAR_MONT_LE; points: n x 64 B MSM_AMD_POINT_H2C_AFFINE;
 * out: 96 B Jacobian (x, y, z) Montgomery LE, normalised to z = R mod p, or z = 0 for the identity:
 * memcpy-compatible with bn256::G1 / G1Projective.
 * A call of 2^19 points or more with nothing else in flight is executed as a pipelined batch of 2 / 4 / 8 point
 * ranges (upload and sort of one range under the bucket accumulation of the previous one) whose results are added
 * on the host -- same result, 17-38 % less wall time; every single-instance entry point does this (device-resident
 * inputs from 2^23 points). */
int msm_amd_gpu_msm_h2c(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, void* out96);
/* gpu_msm_h2c_sync(scalars, points, sync_pair: Arc<(Mutex<bool>, Condvar)>) (msm.rs:237-349): the same MSM, and
 * `after_sort(user)` is called once, on the calling thread, as soon as the sort stage of this MSM has finished on
 * the GPU -- the point where the reference sets the flag and notifies the condvar (msm.rs:306-312) so that a
 * hybrid caller may start its CPU half (gpu_with_cpu, msm.rs:403-415).  after_sort may be NULL.  The callback must
 * not call into the same ctx. */
typedef void (*msm_amd_after_sort_fn)(void* user);
int msm_amd_gpu_msm_h2c_sync(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n,
                             msm_amd_after_sort_fn after_sort, void* user, void* out96);
/* metal_msm::<ArkG, ArkFr>(points, scalars, &mut config) -> Result<ArkG, MetalError> (msm.rs:220-234).
 * points: n x 96 B MSM_AMD_POINT_ARK_PROJECTIVE; scalars: n x 32 B MSM_AMD_SCALAR_MONT_LE. */
int msm_amd_metal_msm_ark(msm_amd_ctx* ctx, const void* points, const void* scalars, size_t n, void* out96);
/* Generic form of the two above with explicit layouts. */
int msm_amd_msm(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* scalars, const void* points,
                size_t n, void* out96);
/* The instance loop of gpu_profiler / benches (gpu_profiler.rs:104-106, msm_benchmark.rs:29-34):
 * n_inst independent MSMs; out = n_inst x 96 B.  Instance i + 1 is uploaded while instance i computes.  With
 * MSM_AMD_POINT_PREPARED / MSM_AMD_POINT_TABLES the points array holds device pointers / table handles (see
 * below) and only the scalars are uploaded. */
int msm_amd_msm_batch(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                      const void* const* scalars, const void* const* points, const size_t* n, void* out);

/* Page-lock a caller buffer so that the host-buffer entry points above upload it by DMA at PCIe rate and without
 * blocking the calling thread (pageable memory is staged by the runtime at about half that rate).  Meant for
 * long-lived inputs such as the bases of an SRS, which the reference re-uploads on every call (msm.rs:152-153).
 * The memory must stay valid and in place until msm_amd_host_unregister (or msm_amd_destroy). */
int msm_amd_host_register(msm_amd_ctx* ctx, const void* ptr, size_t bytes);
int msm_amd_host_unregister(msm_amd_ctx* ctx, const void* ptr);

/* Resident-bases speed for drop-in callers, without an API change (opt-in).  The reference's callers hand over the
 * SAME bases slice on every call (benches/msm_benchmark.rs:116-121) and the reference re-uploads and re-converts it
 * every time (msm.rs:152-153).  With a cache budget of max_bytes > 0 (or MSM_AMD_BASES_CACHE_MB at msm_amd_init) the
 * host-slice entry points -- msm_amd_gpu_msm_h2c, msm_amd_msm, msm_amd_msm_batch, msm_amd_metal_msm_ark,
 * msm_amd_msm_best -- keep the converted device copy of every points array they see (64 B per point, least recently
 * used arrays make way) and on the next call with the same (pointer, n, layout) upload the scalars only.
 * Contract: an array handed over at an unchanged address holds unchanged bases.  As a safety net every hit re-hashes
 * ~2 k sampled records of the caller's memory (record i belongs to phase i mod (n / 1024); phase 0 and one rotating
 * phase are checked per call): a changed array is detected at once if the change touches phase 0, within n / 1024
 * calls otherwise, and is then re-uploaded.  max_bytes = 0 switches the cache off and frees it.
 * stats: [0] hits, [1] misses (entries filled), [2] invalidations (checksum mismatch), [3] bytes held, [4] entries. */
int msm_amd_set_bases_cache(msm_amd_ctx* ctx, size_t max_bytes);
int msm_amd_bases_cache_stats(msm_amd_ctx* ctx, uint64_t stats[5]);
/* A caller that DOES change bases in place says so: the entries of the array at host_points (NULL: all entries) are
 * dropped, the next call uploads again.  This is the contract's other half; the sampling above is only a net. */
int msm_amd_bases_cache_invalidate(msm_amd_ctx* ctx, const void* host_points);
/* full != 0 (or MSM_AMD_BASES_CACHE_VERIFY=full at msm_amd_init): every hit re-hashes EVERY record of the caller's
 * array (64 contiguous slices on four host threads, ~1.5 ms per 2^20 points) before the cached copy is used -- no
 * stale window at all, at about the cost of the upload the cache saves (the conversion is still saved).  0: sampling. */
int msm_amd_set_bases_cache_verify(msm_amd_ctx* ctx, int full);

/* ---- hybrid front-end ----------------------------------------------------------------------- */
/* msm_best::<G1Affine, ..>(scalars, points) -> G1 (msm.rs:424-445): filter_zeros (drop zero scalars when at
 * least 30 % of them are zero, msm.rs:448-507, done here by a device compaction) and then the MSM.  The
 * reference sends n < 2^17 to halo2curves on the CPU because its Metal path is slower there (msm.rs:440-444);
 * the same dispatch exists here with the threshold measured on MI355X: below msm_amd_cpu_dispatch_below()
 * points one blocking GPU call costs more than the product's host bucket method (host_msm, the CPU half of
 * gpu_with_cpu), so those sizes are computed on the host -- an explicit size dispatch as in the reference,
 * never a fallback: without a GPU this entry point fails like every other.  h2c layouts. */
int msm_amd_msm_best(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, void* out96);
/* msm_best's size threshold (the reference's is 2^17, msm.rs:440): sizes below it go to the host bucket method. */
size_t msm_amd_cpu_dispatch_below(void);
/* gpu_with_cpu (msm.rs:366-421): the first split_at points go to the GPU, the rest to a multi-threaded host
 * bucket method (cpu_threads <= 0: all hardware threads); the two results are added.  h2c layouts. */
int msm_amd_gpu_with_cpu(msm_amd_ctx* ctx, const void* scalars, const void* points, size_t n, size_t split_at,
                         int cpu_threads, void* out96);
/* The reference's split policy (msm.rs:377-383): n/3 below 2^18, n/2 below 2^20, else 2n/3 go to the GPU.
 * On MI355X the throughput-optimal split is split_at = n; the policy is kept for parity. */
size_t msm_amd_reference_split(size_t n);
/* The split measured on MI355X: the whole instance goes to the GPU (split_at = n) unless it is smaller than
 * msm_amd_cpu_dispatch_below() -- a CPU share only lengthens the call on this hardware. */
size_t msm_amd_tuned_split(size_t n);
/* The CPU MSM of the library by itself (no ctx, no GPU): what `gpu_profiler <log> <n> cpu` runs where the reference
 * runs halo2curves::msm::msm_best (gpu_profiler.rs:157-159).  Multi-threaded signed-digit Pippenger with
 * batched-affine bucket additions on 4 x 64-bit limbs; h2c affine points, scalars MONT_LE or CANON_LE;
 * threads <= 0: msm_amd_host_threads().  out96 as every other entry point (normalised Jacobian). */
int msm_amd_host_msm(int scalar_layout, int point_layout, const void* scalars, const void* points, size_t n, int threads,
                     void* out96);
/* CPUs the process may really use: affinity mask capped by the cgroup CPU quota. */
int msm_amd_host_threads(void);

/* ---- whole-MSM entry points: inputs already resident in device memory ------------------------ */
/* Same as msm_amd_msm / msm_amd_msm_batch but scalars/points are device pointers on ctx's device
 * (the reference re-uploads and re-converts per call, msm.rs:152-153; an SRS is uploaded once here). */
int msm_amd_msm_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* d_scalars,
                       const void* d_points, size_t n, void* out96_host);
int msm_amd_msm_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                             const void* const* d_scalars, const void* const* d_points, const size_t* n,
                             void* out_host);

/* Pipelined form of msm_amd_msm_batch_device: submit enqueues all GPU work of the batch and returns a ticket;
 * wait finishes it (host Horner pass) and fills out_host (n_inst x 96 B, must stay valid until then).  Up to 4
 * batches may be in flight, so the front end of batch k+1 runs under the accumulation of batch k and the host
 * work of batch k under the GPU work of batch k+1.  The d_scalars / d_points / n arrays (the pointer lists) are read
 * at submit.  The device buffers they name are another matter: the point buffers of every layout -- the caller's own
 * MSM_AMD_POINT_H2C_AFFINE array as much as a prepared array or a table -- are gathered by the accumulate kernel itself
 * and are READ UNTIL THE BATCH HAS BEEN WAITED FOR (msm_amd_wait_batch, or the return of a blocking call); do not free or
 * overwrite them before.  They are never written. */
int msm_amd_submit_batch_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                void* out_host, int* ticket);
int msm_amd_wait_batch(msm_amd_ctx* ctx, int ticket);

/* ---- scalars of bounded width ------------------------------------------------------------------
 * Witness vectors, lookup multiplicities, selector columns and folding challenges are short: bits, bytes, 32 / 64-bit
 * words, 128-bit challenges, and "small negatives" r - k.  A bounded call plans for `bits` bits instead of 254:
 * bits / c + 1 digit windows are extracted, sorted, accumulated and reduced, and the window is the one measured for that
 * width (msm_amd_auto_window_size_bounded).
 * Value and sign: the value of a record is its residue s mod r (MSM_AMD_SCALAR_MONT_LE records are de-Montgomeryed,
 * raw MSM_AMD_SCALAR_CANON_* words reduced first, as everywhere).  MSM_AMD_WIDTH_UNSIGNED: the magnitude is s.
 * MSM_AMD_WIDTH_SIGNED: the magnitude is min(s, r - s) and the record counts as negative when s > (r - 1) / 2 (its
 * point is subtracted).  bits: 1..254 unsigned, 1..253 signed (a signed bound of 253 takes every residue); anything
 * else, or another sign, is MSM_AMD_INPUT_ERROR.
 * Contract: the result is the group element, and so the bytes, of the unbounded call on the same inputs.  A record whose
 * magnitude is 2^bits or more makes the call return MSM_AMD_INPUT_ERROR after its GPU work: msm_amd_last_error gives the
 * number of such records and the index of the first of them (and the instance, for a batch; for a call the library cut
 * into point ranges the count is that of the first violating range), the output is left untouched and the ctx stays
 * usable -- a wrong result is never returned.  A bound of 254 unsigned is the unbounded call.
 * What it buys (one MI355X, profiles/bounded_bench.json): every width from 8 to 128 bits is faster than the unbounded call
 * on the same scalars at 2^16, 2^20 and 2^22 points, 8-bit values 5 - 12x from 2^20 points, +-small values up to 18x.
 * Scalars of ONE or two bits are the exception: every point lands in the same bucket, which is cut into thousands of
 * work items and summed by the combine pass, and from 2^20 points the unbounded call (whose other windows keep the
 * work items long) is up to 2.4x faster -- keep boolean vectors on msm_amd_msm* (DESIGN.md section 8.10). */
enum { MSM_AMD_WIDTH_UNSIGNED = 0, MSM_AMD_WIDTH_SIGNED = 1 };
/* The width of a vector: *bits = the largest bit length of a magnitude (0 for an all-zero vector and for n == 0);
 * stats (optional, 4 words): zero records, negative records (signed only), the lowest index of a widest record, 0.
 * Scalars: MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE, host memory / device memory (_device), n < 2^32.  One
 * pass over the records and a fold of per-wave partials; a blocking call like the Fr vector calls.  Scan a circuit's
 * witness once, then commit with msm_amd_msm_bounded_device at that width. */
int msm_amd_scalar_width(msm_amd_ctx* ctx, int scalar_layout, const void* scalars, size_t n, int sign, uint32_t* bits,
                         uint64_t stats[4]);
int msm_amd_scalar_width_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_scalars, size_t n, int sign,
                                uint32_t* bits, uint64_t stats[4]);
/* Host twin (no ctx, no GPU); threads <= 0: up to 16 host threads. */
int msm_amd_host_scalar_width(int scalar_layout, const void* scalars, size_t n, int sign, int threads, uint32_t* bits,
                              uint64_t stats[4]);
/* msm_amd_msm / msm_amd_msm_device / msm_amd_msm_batch_device / msm_amd_submit_batch_device at a bounded width; every
 * point layout of the unbounded form, MSM_AMD_POINT_PREPARED and MSM_AMD_POINT_TABLES included (a table is used through
 * its first bits / c + 1 windows, at the table's c).  One bits / sign for a whole batch; a ticket is collected by
 * msm_amd_wait_batch, which reports a violated bound. */
int msm_amd_msm_bounded(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* scalars, const void* points,
                        size_t n, uint32_t bits, int sign, void* out96);
int msm_amd_msm_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, const void* d_scalars,
                               const void* d_points, size_t n, uint32_t bits, int sign, void* out96_host);
int msm_amd_msm_batch_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                     const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                     uint32_t bits, int sign, void* out_host);
int msm_amd_submit_batch_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout, size_t n_inst,
                                        const void* const* d_scalars, const void* const* d_points, const size_t* n,
                                        uint32_t bits, int sign, void* out_host, int* ticket);
/* The CPU MSM at that width (msm_amd_host_msm): MSM_AMD_INPUT_ERROR, output untouched, for a record beyond the bound. */
int msm_amd_host_msm_bounded(int scalar_layout, int point_layout, const void* scalars, const void* points, size_t n,
                             uint32_t bits, int sign, int threads, void* out96);
/* The window a bounded call of n points uses (lone != 0: one instance with nothing else in flight); bits = 254 gives
 * msm_amd_auto_window_size / msm_amd_auto_window_size_lone.  msm_amd_set_window_size overrides it.  Measured on MI355X
 * from 2^16 to 2^22 points (profiles/bounded_sweep.txt): up to 16 bits ONE window that holds the whole scalar
 * (c = bits + 1); above, the fewest windows whose top digit is wide enough that no bucket outgrows a work item (32 and 64
 * bits: c = 17; 128 bits: c = 10 from 2^19 points), and c <= 13 for instances up to 2^18 points that need four windows
 * or more or run pipelined at 2^16.  Below 2^15 points: the window of the unbounded call. */
uint32_t msm_amd_auto_window_size_bounded(size_t n, uint32_t bits, int lone);

/* Upper bound of every host wait for the GPU inside the library, in milliseconds (default 60 000, or the environment
 * variable MSM_AMD_WAIT_TIMEOUT_MS at msm_amd_init; 0 = wait without bound).  The reference's gpu_msm_h2c_sync is one
 * blocking call that always returns (msm.rs:237-349); so is every call here: a wait that reaches the bound returns
 * MSM_AMD_PIPELINE_ERROR and msm_amd_last_error names the stage event and the instance the device did not reach.
 * The work stays in flight: a ticket of msm_amd_submit_batch_device stays valid and may be waited for again; after a
 * blocking entry point timed out, the next call first checks whether the device has caught up (and fails the same
 * way if not); msm_amd_synchronize waits once more; msm_amd_destroy gives the device resources up rather than
 * freeing memory under running kernels.
 * The same bound covers memory management: the library never calls hipMalloc / hipHostMalloc / hipFree / hipHostFree
 * while the ctx has work in flight (they may wait for the device, hipFree always does).  A call that has to GROW a
 * workspace, a page-locked result slot or the staging ring first waits -- bounded -- for the ctx's streams to run
 * empty and returns MSM_AMD_PIPELINE_ERROR ("device busy ... cannot grow") if they do not; buffers that are outgrown
 * or dropped (bases cache entries, msm_amd_device_free on a busy ctx) are released when the ctx is idle again.
 * After a timeout, host buffers the caller registered with msm_amd_host_register may still be read by DMA: keep
 * them alive until msm_amd_synchronize has returned MSM_AMD_OK. */
int msm_amd_set_wait_timeout_ms(msm_amd_ctx* ctx, uint32_t timeout_ms);

/* ---- several GPUs ---------------------------------------------------------
 * The instance loop of the reference (gpu_profiler.rs:101-106, benches/msm_benchmark.rs:29-34) sharded over
 * several ctxs: instance j runs on ctxs[j mod n_ctx], one host thread per ctx (pinned to the CPUs local to the
 * ctx's GPU when sysfs exposes them), no data-path collective; results land at out + 96 j.  The ctxs may sit on
 * different GPUs (the intended use) or on one (they then share it).  _multi takes host buffers like
 * msm_amd_msm_batch; _multi_device takes device buffers, those of instance j on the device of ctxs[j mod n_ctx].
 * On failure the first failing ctx's status is returned and msm_amd_last_error(that ctx) has the detail. */
int msm_amd_msm_batch_multi(msm_amd_ctx* const* ctxs, size_t n_ctx, int scalar_layout, int point_layout, size_t n_inst,
                            const void* const* scalars, const void* const* points, const size_t* n, void* out);
int msm_amd_msm_batch_multi_device(msm_amd_ctx* const* ctxs, size_t n_ctx, int scalar_layout, int point_layout,
                                   size_t n_inst, const void* const* d_scalars, const void* const* d_points,
                                   const size_t* n, void* out_host);
/* Pipelined form of msm_amd_msm_batch_multi_device (the multi-ctx twin of msm_amd_submit_batch_device /
 * msm_amd_wait_batch): submit enqueues every ctx's share and returns a ticket, wait finishes all shares and writes
 * out_host + 96 j (out_host must stay valid until then).  Up to 4 batches may be in flight per ctx, so a caller
 * looping over batches -- benches/msm_benchmark.rs:29-34 -- keeps every GPU busy across calls.  wait frees the ticket
 * on success; after a bounded-wait timeout (MSM_AMD_PIPELINE_ERROR, work still in flight) the ticket stays valid. */
typedef struct msm_amd_multi_ticket msm_amd_multi_ticket;
int msm_amd_submit_batch_multi_device(msm_amd_ctx* const* ctxs, size_t n_ctx, int scalar_layout, int point_layout,
                                      size_t n_inst, const void* const* d_scalars, const void* const* d_points,
                                      const size_t* n, void* out_host, msm_amd_multi_ticket** ticket);
int msm_amd_wait_batch_multi(msm_amd_multi_ticket* ticket);
/* ONE instance of n points over several ctxs, split by point range ("single huge instance"):
 * ctx g uploads and runs the MSM of points [begin_g, end_g) (msm_amd_shard_range), the partial results are added with
 * msm_amd_sum_points -- the algebra of the reference's GPU + CPU split, src/metal/msm.rs:385-419.  Host buffers in a
 * host layout (not MSM_AMD_POINT_PREPARED / _TABLES, which belong to one ctx); out96 as msm_amd_msm. */
int msm_amd_msm_range_multi(msm_amd_ctx* const* ctxs, size_t n_ctx, int scalar_layout, int point_layout,
                            const void* scalars, const void* points, size_t n, void* out96);
void msm_amd_shard_range(size_t n, size_t n_ctx, size_t k, size_t* begin, size_t* end);
/* Bytes per element of a layout (0 = unknown layout). */
size_t msm_amd_scalar_bytes(int scalar_layout);
size_t msm_amd_point_bytes(int point_layout);
/* The sharding arithmetic: owner of instance j, and how many instances ctx k of n_ctx gets. */
size_t msm_amd_shard_owner(size_t instance, size_t n_ctx);
size_t msm_amd_shard_count(size_t n_inst, size_t n_ctx, size_t k);
/* HIP device ordinal of a ctx. */
int msm_amd_ctx_device(const msm_amd_ctx* ctx);
/* Restrict the calling thread to the CPUs local to `device` (sysfs local_cpulist of its PCI function, intersected
 * with the thread's current mask).  0 = pinned, 1 = no NUMA information or fewer than 8 CPUs to intersect (not an
 * error; the mask is left alone). */
int msm_amd_pin_thread_to_device(int device);

/* RCCL all-gather of per-rank result blocks (one communicator per listed device, created in this process with
 * ncclCommInitAll; librccl is loaded on first use, not linked).  send_host[k] = rank k's bytes_per_rank bytes
 * (its ceil(I / G) x 96 B of results), recv_host[k] = n_devices x bytes_per_rank bytes, every rank's block in rank
 * order, moved through rank k's GPU over xGMI.  A deployment with one PROCESS per GPU does the same with its own
 * communicator (bench.py: torch.distributed, backend nccl = RCCL). */
typedef struct msm_amd_gather msm_amd_gather;
int msm_amd_gather_init(const int* devices, int n_devices, msm_amd_gather** out);
int msm_amd_gather_size(const msm_amd_gather* g);
int msm_amd_gather_all(msm_amd_gather* g, const void* const* send_host, size_t bytes_per_rank, void* const* recv_host);
const char* msm_amd_gather_last_error(const msm_amd_gather* g);
void msm_amd_gather_destroy(msm_amd_gather* g);

/* ---- persistent bases -----------------------------------------------------------------------
 * The reference converts and re-uploads the bases on every call (msm.rs:152-153); provers reuse one SRS for
 * many MSMs.  These calls convert a point array once into the library's internal 64-byte form, resident on the
 * device; pass the result as d_points with MSM_AMD_POINT_PREPARED to the *_device entry points, or use
 * msm_amd_msm_prepared with host scalars.  Prepared arrays are freed with msm_amd_device_free. */
int msm_amd_bases_upload(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, void** d_prepared);
int msm_amd_bases_prepare_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n,
                                 void* d_prepared /* n x 64 bytes */);
int msm_amd_msm_prepared(msm_amd_ctx* ctx, int scalar_layout, const void* scalars, const void* d_prepared, size_t n,
                         void* out96);

/* ---- partial results ------------------------------------------------------------------------
 * Host-side sum of `count` results (96 B Jacobian Montgomery LE each, as every entry point above returns
 * them), normalised like them.  It is the final addition of gpu_with_cpu (msm.rs:418-419) made available to
 * callers that split ONE instance by point range across several GPUs: every rank runs the MSM of its range,
 * the 96-byte partial results are all-gathered, and every rank adds them. */
int msm_amd_sum_points(const void* points96, size_t count, void* out96);

/* ---- precomputed window tables (fixed bases) ---------------------------------------------------
 * Beyond the reference: for a fixed set of bases (an SRS) the library can store 2^(c w) P_i for every window w
 * (W x n x 64 bytes; 0.9 GB for 2^20 points -- HBM is 288 GB).  All windows then share ONE set of 2^(c-1)
 * buckets, so the window grows to c = log2(n) - 1 and an MSM needs ~18 % fewer point additions at 2^20 points,
 * with the same results bit for bit.  Build once (about 0.1 s per 2^20 points), then pass the handle as the points
 * pointer with MSM_AMD_POINT_TABLES to the *_device entry points (n must equal the table's n), or call
 * msm_amd_msm_tables with host scalars.  window_size 0 = automatic. */
typedef struct msm_amd_tables msm_amd_tables;
int msm_amd_tables_build(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, uint32_t window_size,
                         msm_amd_tables** out);
int msm_amd_tables_build_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n,
                                uint32_t window_size, msm_amd_tables** out);
int msm_amd_tables_info(msm_amd_ctx* ctx, const msm_amd_tables* tables, size_t* n, uint32_t* window_size,
                        uint32_t* num_windows, size_t* device_bytes);
int msm_amd_tables_free(msm_amd_ctx* ctx, msm_amd_tables* tables);
int msm_amd_msm_tables(msm_amd_ctx* ctx, const msm_amd_tables* tables, int scalar_layout, const void* scalars,
                       void* out96);

/* ---- device memory helpers (so callers without a HIP binding can stage data) ------------------ */
int msm_amd_device_alloc(msm_amd_ctx* ctx, size_t bytes, void** d_ptr);
int msm_amd_device_free(msm_amd_ctx* ctx, void* d_ptr);
int msm_amd_copy_to_device(msm_amd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int msm_amd_copy_to_host(msm_amd_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* Raw hipStream_t of the ctx (for event/stream interop from torch or HIP callers). */
void* msm_amd_stream(msm_amd_ctx* ctx);
int msm_amd_synchronize(msm_amd_ctx* ctx);

/* Deterministic synthetic instance on the device (role of preprocess.rs:113-138): n uniform random
 * G1 points (64 B affine, Montgomery) and n uniform scalars (Montgomery if scalars_mont else canonical LE). */
int msm_amd_generate_instance(msm_amd_ctx* ctx, uint64_t seed, size_t n, int scalars_mont, void* d_points,
                              void* d_scalars);

/* Unit-test hook of the CPU MSM's AVX-512 IFMA arithmetic (csrc/host_ifma.cpp): count canonical field elements of
 * 4 x u64 LE each.  op 0: a b / 2^260 mod p; 1: a - b mod p; 2: -a mod p (a != 0); 3: a 2^4 mod p (R -> Q domain);
 * 4: a / 2^4 mod p (Q -> R).  MSM_AMD_FUNCTION_ERROR on a host without IFMA. */
int msm_amd_test_op_ifma(int op, const void* a, const void* b, void* out, size_t count);
/* The same instance generated on the host (identical bytes; no ctx, no GPU): inputs of `gpu_profiler ... cpu`. */
int msm_amd_generate_instance_host(uint64_t seed, size_t n, int scalars_mont, void* points, void* scalars, int threads);

/* ---- instance files (src/utils/preprocess.rs:30-111, 143-212) -------------------------------------
 * The reference caches benchmark inputs as bincode 1.3 `Vec<(Vec<Vec<u32>>, Vec<Vec<u32>>)>`:
 *   u64 n_instances; per instance { u64 n_points; n_points x { u64 24; u32 x 24 };
 *                                   u64 n_scalars; n_scalars x { u64 8; u32 x 8 } }     (all little-endian)
 * with points in MSM_AMD_POINT_JAC_BE32 and scalars in MSM_AMD_SCALAR_CANON_BE32, under the name
 * msm_{log_size}x{num_instances}.bin.  These host-only functions read and write that format, so that
 * files interchange with the reference's ~/.msm_gpu_acceleration/msm_vecs cache.  No ctx and no GPU needed. */
typedef struct msm_amd_instance_file msm_amd_instance_file;

/* save_msm_instances (preprocess.rs:84-97): points[j] = n[j] x 96 B (JAC_BE32), scalars[j] = n[j] x 32 B
 * (CANON_BE32). */
int msm_amd_instances_save(const char* path, size_t n_inst, const size_t* n, const void* const* points,
                           const void* const* scalars);
/* load_msm_instances (preprocess.rs:99-111), streaming: open scans the record structure only. */
int msm_amd_instances_open(const char* path, msm_amd_instance_file** out);
size_t msm_amd_instances_count(const msm_amd_instance_file* f);
size_t msm_amd_instances_size(const msm_amd_instance_file* f, size_t j);   /* points (= scalars) of instance j */
int msm_amd_instances_read(msm_amd_instance_file* f, size_t j, void* points_out, void* scalars_out);
void msm_amd_instances_close(msm_amd_instance_file* f);
/* msm_{log}x{n}.bin under dir, or under $HOME/.msm_gpu_acceleration/msm_vecs when dir is NULL
 * (preprocess.rs:165, 204-212).  Returns the length written (without the NUL), 0 if buf is too small. */
size_t msm_amd_instances_default_path(const char* dir, uint32_t log_size, uint32_t num_instances, char* buf,
                                      size_t buf_len);
/* Host layout conversion between a caller layout and the wire layout (role of the ToLimbs / FromLimbs
 * impls, limbs_conversion.rs:87-195, 282-389).  to_wire accepts every scalar and point layout; an affine
 * identity becomes z = 0.  from_wire produces MSM_AMD_SCALAR_{MONT_LE,CANON_LE} and
 * MSM_AMD_POINT_ARK_PROJECTIVE (a limb reorder: coordinates are not normalised). */
int msm_amd_to_wire(int scalar_layout, int point_layout, const void* scalars, const void* points, size_t n,
                    void* scalars_be32_out, void* points_be32_out);
int msm_amd_from_wire(int scalar_layout, int point_layout, const void* scalars_be32, const void* points_be32,
                      size_t n, void* scalars_out, void* points_out);

/* ---- per-stage entry points in the reference's wire layout (host buffers) ---------------------
 * These are the `pub` stage functions the reference's own stage tests drive through
 * create_test_instance (sort_buckets.rs:38-69, bucket_wise_accumulation.rs:154-224,
 * sum_reduction.rs:210-258). u32 limbs are most-significant-first (MSM_AMD_*_BE32). */
/* prepare_buckets_indices (prepare_buckets_indices.rs:15-38 + msm.h.metal:17-59): scalars n x 8 u32
 * canonical BE32 -> pairs n*W x 2 u32 at [t*W + i] = (i*(2^c-1) + m - 1, t) or (0xFFFFFFFF,0xFFFFFFFF). */
int msm_amd_prepare_buckets_indices(msm_amd_ctx* ctx, const uint32_t* scalars_be32, size_t n, uint32_t window_size,
                                    uint32_t num_windows, uint32_t* pairs_out);
/* sort_buckets_indices (sort_buckets.rs:15-34): sort n_pairs (u32,u32) pairs by .0 ascending, in place. */
int msm_amd_sort_buckets_indices(msm_amd_ctx* ctx, uint32_t* pairs, size_t n_pairs);
/* The same sort on a device-resident buffer, in place (the measured form of the stage: what
 * benches/sort_buckets_indices_benchmark.rs:10-32 times around the reference's CPU sort).  Only the low
 * key_bits bits of the key are sorted on (32 = full keys incl. the 0xFFFFFFFF sentinels; 8 bits per pass).
 * kernel_ms (optional) receives the device time of the sort. */
int msm_amd_sort_pairs_device(msm_amd_ctx* ctx, void* d_pairs, size_t n_pairs, uint32_t key_bits, float* kernel_ms);
/* bucket_wise_accumulation (bucket_wise_accumulation.rs:26-107): pairs sorted by bucket; points
 * n_points x 24 u32 Jacobian BE32; buckets_out total_buckets x 24 u32 (untouched buckets = all zero,
 * i.e. z = 0, as Metal's zero-filled buffers give the reference). */
int msm_amd_bucket_wise_accumulation(msm_amd_ctx* ctx, const uint32_t* sorted_pairs, size_t n_pairs,
                                     const uint32_t* points_be32, size_t n_points, uint32_t total_buckets,
                                     uint32_t* buckets_out);
/* sum_reduction (sum_reduction.rs:161-181): res[j] = sum_b (b+1) * buckets[j*buckets_size + b]. */
int msm_amd_sum_reduction(msm_amd_ctx* ctx, const uint32_t* buckets_be32, uint32_t buckets_size,
                          uint32_t num_windows, uint32_t* res_out);
/* final_accumulation (final_accumulation.rs:5-40): Horner over the window sums, on the host. */
int msm_amd_final_accumulation(const uint32_t* res_be32, uint32_t num_windows, uint32_t window_size,
                               uint32_t* point_out);

/* ---- single-op test kernels (role of the kernels in shader/tests/ and curves/bn254.h.metal) ------------
 * Batched: `count` independent operations, one lane each.  Operands are 8 x u32 BE32 limbs per 256-bit
 * value; points are 24 x u32. */
enum {
  MSM_AMD_OP_UINT_ADD = 0,  /* test_uint_add   a + b mod 2^256 */
  MSM_AMD_OP_UINT_SUB = 1,  /* test_uint_sub */
  MSM_AMD_OP_UINT_PROD = 2, /* test_uint_prod  a * b[low 32 bits] mod 2^256 */
  MSM_AMD_OP_UINT_SHL = 3,  /* test_uint_shl   a << (b mod 256) */
  MSM_AMD_OP_UINT_SHR = 4,  /* test_uint_shr */
  MSM_AMD_OP_FP_ADD = 5,    /* fp_bn254_add (Montgomery residues in and out) */
  MSM_AMD_OP_FP_SUB = 6,
  MSM_AMD_OP_FP_MUL = 7,
  MSM_AMD_OP_FP_NEG = 8,
  MSM_AMD_OP_FP_POW = 9,    /* a ^ (b low 32 bits) */
  MSM_AMD_OP_EC_ADD = 10,   /* bn254_add: Jacobian + Jacobian; a, b, out are 24 limbs */
  MSM_AMD_OP_EC_MUL = 11,   /* bn254_scalar_mul: a = point (24 limbs), b = scalar (8 limbs, canonical) */
  MSM_AMD_OP_EC_MADD = 12,  /* Jacobian a + affine b (b given as 24 limbs with z = one or z = 0) */
  MSM_AMD_OP_EC_DBL = 13,   /* 2 * a */
  /* ops of the 29-bit-limb internal representation the hot kernels compute in (csrc/bn254_fq29.hip.h);
   * operands and results cross the boundary in the same external form as above */
  MSM_AMD_OP_FP29_MUL = 14,
  MSM_AMD_OP_FP29_SQR = 15,
  MSM_AMD_OP_FP29_SUB_K4E30 = 16,  /* a - b through the lifted constant 4p */
  MSM_AMD_OP_FP29_SUB_K8E30 = 17,
  MSM_AMD_OP_FP29_SUB_K8E31 = 18,  /* a - 3b (lazy three-term subtrahend) */
  MSM_AMD_OP_FP29_SUB_K16E30 = 19,
  MSM_AMD_OP_FP29_SUB_K16E31 = 20, /* a - 3b */
  MSM_AMD_OP_FP29_ROUNDTRIP = 21,  /* external -> internal -> external */
  MSM_AMD_OP_EC29_MADD = 22,       /* Jacobian a + affine b on internal limbs */
  MSM_AMD_OP_EC29_ADD = 23,        /* Jacobian a + Jacobian b on internal limbs */
  MSM_AMD_OP_EC29_MADD_CHAIN = 24, /* a + 64 b: 64 chained mixed additions kept in the lazy internal form */
  MSM_AMD_OP_EC29_ADD_CHAIN = 25,  /* a + 16 b: 16 chained full additions */
  MSM_AMD_OP_EC29_MMADD = 26,      /* -a - 4b: affine + affine (4M + 2S start of a work item) on lazily negated
                                      operands, then three mixed additions; a, b finite with z = one */
  /* host only (msm_amd_test_op_host; msm_amd_test_op rejects them): the 4 x 64-bit arithmetic of the CPU tail of
     every MSM -- window Horner pass and normalisation (csrc/host_fq64.h) */
  MSM_AMD_OP_H64_FP_MUL = 27,
  MSM_AMD_OP_H64_FP_ADD = 28,
  MSM_AMD_OP_H64_FP_SUB = 29,
  MSM_AMD_OP_H64_EC_ADD = 30,      /* Jacobian + Jacobian, 24 limbs each */
  MSM_AMD_OP_H64_EC_DBL = 31,
  /* field ops on internal limbs again (device and host): build options of the multiplication that were measured and
     not shipped -- one Karatsuba level, lockstep product-scanning chains; operands / results as for op 14 */
  MSM_AMD_OP_FP29_MUL_KARATSUBA = 32, /* a * b */
  MSM_AMD_OP_FP29_LOCKSTEP_PAIR = 33, /* a * b + b * b        (two products side by side) */
  MSM_AMD_OP_FP29_LOCKSTEP_MIX = 34,  /* 2 a b + 2 a^2 + b^2  (double product next to a product, squaring pair) */
  MSM_AMD_OP_FP29_LOCKSTEP_TRIPLE = 35, /* a b + a^2 + b^2    (three products side by side) */
  MSM_AMD_OP_FP29_MUL2_KARATSUBA = 36, /* 2 a b               (schoolbook + Karatsuba product, one reduction) */
  /* host only again: the inversion of the CPU tail (normalisation of every result, batched-affine CPU MSM) */
  MSM_AMD_OP_H64_FP_INV = 37,        /* a^-1 by the binary GCD with 31-step rounds; 0 -> 0; b ignored */
  MSM_AMD_OP_H64_FP_INV_FERMAT = 38  /* a^(p-2), its checker */
};
int msm_amd_test_op(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);
/* The same operation bodies executed on the host CPU (no GPU needed): host-logic tests. */
int msm_amd_test_op_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);

/* ---- raw-limb test ops of the 29-bit-limb internal representation (csrc/bn254_fq29.hip.h, bn254_ec29.hip.h) -----
 * The limbs pass through exactly as given: no from_ext, no byte reversal, no normalisation in or out, so that a test
 * can put operands at the edges of the bounds contract and read result limbs.  Fixed-width records: a and b are 36
 * little-endian u32 per element, out is 40.  a0 / a1 (b0 / b1) are words 0..8 / 9..17 of a (b); a point (PtI) is
 * X, Y, ZZ, ZZZ in 36 words, an affine base (AffI) x, y in 18.  count <= 2^24; unknown ops: MSM_AMD_INPUT_ERROR. */
enum {
  MSM_AMD_RAW_FE_MUL = 0,        /* out[0..8] = mul(a0, b0) */
  MSM_AMD_RAW_FE_SQR = 1,        /* sqr(a0) */
  MSM_AMD_RAW_FE_MUL2 = 2,       /* mul2(a0, a1, b0, b1) = a0 a1 + b0 b1, one reduction */
  MSM_AMD_RAW_FE_SUB_K4E30 = 3,  /* sub<K>(a0, b0) = a0 + K - b0, not normalised */
  MSM_AMD_RAW_FE_SUB_K8E30 = 4,
  MSM_AMD_RAW_FE_SUB_K8E31 = 5,
  MSM_AMD_RAW_FE_SUB_K16E30 = 6,
  MSM_AMD_RAW_FE_SUB_K16E31 = 7,
  MSM_AMD_RAW_FE_NORM = 8,
  MSM_AMD_RAW_FE_NEG = 9,
  MSM_AMD_RAW_FE_NEG_WIDE = 10,
  MSM_AMD_RAW_FE_CANONICAL = 11, /* canonical(a0, rounds = min(b0[0], 64)) */
  MSM_AMD_RAW_FE_TO_EXT = 12,    /* out[0..7] = to_ext(a0), little-endian */
  MSM_AMD_RAW_FE_PACK_UNPACK = 13, /* out[0..8] = unpack256(pack256(a0)), out[9..16] = pack256(a0) */
  MSM_AMD_RAW_FE_ZERO = 14,      /* out[0] = maybe_zero(a0, bound = b0[0]), out[1] = is_zero_exact(a0) */
  MSM_AMD_RAW_PT_MADD = 15,      /* out[0..35] = PtI a + AffI b (pti_madd_head + pti_madd_tail), out[36] = vanished */
  MSM_AMD_RAW_PT_MMADD = 16,     /* affine (a0, a1) + AffI b (pti_mmadd_head + pti_mmadd_tail), out[36] = vanished */
  MSM_AMD_RAW_PT_ADD_NZ = 17,    /* PtI a + PtI b, neither the identity (pti_add_nz), out[36] = vanished */
  MSM_AMD_RAW_PT_ADD = 18,       /* pti_add: identities allowed, out[36] = 0 */
  MSM_AMD_RAW_PT_DOUBLE = 19,    /* pti_double(a) */
  /* the point additions' forms with wide quotient digits (reduce_columns<true>): 20..31 stay unknown */
  MSM_AMD_RAW_FE_MUL_WIDE = 32,  /* mul_np(a0, b0) */
  MSM_AMD_RAW_FE_SQR_WIDE = 33,  /* sqr_np(a0) */
  MSM_AMD_RAW_FE_MUL2_WIDE = 34, /* mul2w_np(a0, a1, b0, b1) */
  /* 35 stays unknown (tests pin it as refused) */
  MSM_AMD_RAW_FE_SQRT = 36,      /* square root of a0 (normalised, < 8 p) by the ladder of the decompression kernels
                                    (csrc/compress_points.hip.h): out[0..8] = root, out[9] = 1 if there is one, else
                                    all zero; b ignored */
  MSM_AMD_RAW_BASES_IN_PLACE = 40,/* external records as the accumulate kernel gathers them in place (the image of
                                    the point on the isomorphic curve E': limbs of x << 3 and y << 2).  a[0..15],
                                    a[16..31], b[1..16]: records 0, 1, 2 (x, y: 8 + 8 words, little-endian); a[32]:
                                    bit k = negate record k; b[0] = 0: out[0..8], out[9..17] = the limbs of record 0,
                                    out[18] = its sixteen words are all zero, out[19..27] = its lazily negated y;
                                    b[0] = 1: out[0..35] = record 0 + record 1 by the affine start, out[36] = vanished;
                                    b[0] = 2: (record 0 + record 1) + record 2 by the mixed addition */
  MSM_AMD_RAW_FE_MUL_SUB = 44,   /* mul_sub_np<K>(a0, a1, b0) = a0 a1 / rho + K - b0, the lifted subtraction folded into
                                    the reduction; K = b1[0]: 0..5 = K4E30, K8E30, K8E31, K16E30, K16E31, K12E30 (any
                                    other: zero limbs) */
  MSM_AMD_RAW_FE_SQR_SUB = 45    /* sqr_sub_np<K>(a0, b0) = a0^2 / rho + K - b0, K = b1[0] */
};
int msm_amd_test_op_raw(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);
/* The same bodies on the host CPU (no GPU needed). */
int msm_amd_test_op_raw_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);

/* Test aid for the bounded waits: keeps the ctx's main stream busy for at most max_ms (<= 5000) or until
 * msm_amd_test_release(handle).  The kernel carries its own time limit. */
int msm_amd_test_hold(msm_amd_ctx* ctx, uint32_t max_ms, void** handle);
int msm_amd_test_release(msm_amd_ctx* ctx, void* handle);

/* Stage tap for tests: the intermediate buffers of the batch the ctx last waited for (a blocking call, or
 * msm_amd_wait_batch), read AFTER the call -- the call itself runs the shipped pipeline unchanged.  Instance j of a
 * batch of at most four instances (the ctx's workspaces are used round-robin); a larger batch: MSM_AMD_INPUT_ERROR.
 * The record stays valid until the next call on the ctx. */
enum {
  MSM_AMD_TP_C = 0, MSM_AMD_TP_W, MSM_AMD_TP_W_DIGITS, MSM_AMD_TP_N, MSM_AMD_TP_N_SCALARS, MSM_AMD_TP_LB, MSM_AMD_TP_NB,
  MSM_AMD_TP_CH, MSM_AMD_TP_HB, MSM_AMD_TP_MB, MSM_AMD_TP_FB, MSM_AMD_TP_Q, MSM_AMD_TP_TILED, MSM_AMD_TP_BALLOT,
  MSM_AMD_TP_WIDE_DIGITS, MSM_AMD_TP_LONE,   /* 1: the call ran as a lone call (one stream, lone-call reduce geometry) */
  MSM_AMD_TP_TOTAL_ITEMS, MSM_AMD_TP_MULTI_COUNT, MSM_AMD_TP_DEFERRED,   /* plan counters; deferred = split buckets
                                                                            summed by combine_big_kernel */
  MSM_AMD_TP_RED_GROUP, MSM_AMD_TP_RB_THREADS, MSM_AMD_TP_INSTANCES, MSM_AMD_TP_WORKSPACE, MSM_AMD_TP_FRONT_THREADS,
  MSM_AMD_TP_FUSED_FRONT,   /* 1: digits and the pass-1 histogram of the sort ran as one kernel (digits_hist_kernel) */
  MSM_AMD_TP_PACKED,        /* 1: sort pass 1 wrote one packed u32 per entry (fine | index << fb | sign << 31) */
  MSM_AMD_TEST_PLAN_WORDS
};
/* out: count >= MSM_AMD_TEST_PLAN_WORDS words, indexed by MSM_AMD_TP_*. */
int msm_amd_test_last_plan(msm_amd_ctx* ctx, uint32_t j, uint32_t* out, size_t count);
/* Buffers of msm_amd_test_stage_copy (W windows, n entries per window, nb = 2^lb slots per window): */
enum {
  MSM_AMD_STAGE_DIGITS = 0,    /* [W_digits][n_scalars] u16 (c <= 15) or u32: sign << (bits - 1) | magnitude */
  MSM_AMD_STAGE_SORTED = 1,    /* [W][n] u32 point index | sign << 31, grouped by slot */
  MSM_AMD_STAGE_BUCKET_SIZE = 2,   /* [W][nb] u32 */
  MSM_AMD_STAGE_BUCKET_START = 3,  /* [W][nb] u32, offset inside the window's slice of SORTED */
  MSM_AMD_STAGE_ITEM_START = 4,    /* [W][nb] u32, first work item of the slot inside its window */
  MSM_AMD_STAGE_WIN_ITEMS = 5,     /* [W] u32, first work item of the window (exclusive scan of the item counts) */
  MSM_AMD_STAGE_ORDER = 6,         /* [total_items] (slot, chunk) u32 pairs, the accumulate kernel's lane order */
  MSM_AMD_STAGE_MULTI_LIST = 7,    /* [multi_count] u32 slots split into more than one work item */
  MSM_AMD_STAGE_BUCKETS = 8,       /* [W][nb] Jacobian BE32 (24 u32); slots with bucket size 0 hold stale data */
  MSM_AMD_STAGE_PARTIAL = 9        /* [W][lb + 1] Jacobian BE32: bit-k subset sums over the slot index, then the total */
};
/* out == NULL: *bytes receives the size of the buffer; otherwise *bytes must equal it. */
int msm_amd_test_stage_copy(msm_amd_ctx* ctx, uint32_t j, int which, void* out, size_t* bytes);
/* Fill the point-valued buffers of every workspace (buckets, item partials, reduce scratch, window partials), those of
 * the G2 MSM included, and the intermediate records and fixed-base tables of the mul_points calls, with one byte over
 * their whole capacity.  Index and count buffers are never touched. */
int msm_amd_test_fill_workspaces(msm_amd_ctx* ctx, uint8_t byte);
/* The same tap for the G2 MSM: the last msm_amd_msm_g2* call of the ctx (per-call, prepared or tables), read AFTER the
 * call.  MSM_AMD_INPUT_ERROR before any G2 MSM has succeeded and after a failed one; G1 calls in between change nothing.
 * The plan words are the MSM_AMD_TP_* ones with LONE = 1, INSTANCES = 1, WORKSPACE = 0.  The index and count buffers
 * have the formats above; MSM_AMD_STAGE_BUCKETS and MSM_AMD_STAGE_PARTIAL are 192-byte records in the result form of
 * msm_amd_msm_g2 (Jacobian, Montgomery LE, not normalised); z all zero = the identity. */
int msm_amd_test_g2_last_plan(msm_amd_ctx* ctx, uint32_t* out, size_t count);
int msm_amd_test_g2_stage_copy(msm_amd_ctx* ctx, int which, void* out, size_t* bytes);

/* ---- BN254 G2 MSM ------------------------------------------------------------------------------ */
/* G2 is the twist y^2 = x^3 + 3 / (9 + u) over Fq2 = Fq[u] / (u^2 + 1); an Fq2 element is c0 then c1, each 32 B
 * Montgomery LE (R = 2^256).  Scalars use the MSM_AMD_SCALAR_* layouts above; inputs are taken as points of the
 * r-torsion subgroup (no subgroup check; msm_amd_g2_check_points below is the check).  The result is 192 B Jacobian, Montgomery LE (x.c0, x.c1, y.c0, y.c1, z.c0,
 * z.c1), normalised to z = (R mod p, 0); the identity is ((R, 0), (R, 0), (0, 0)). */
enum {
  MSM_AMD_G2_POINT_H2C_AFFINE = 0, /* halo2curves bn256::G2Affine {x, y}: 128 B, identity = all zero */
  MSM_AMD_G2_POINT_ARK_AFFINE = 1, /* ark_bn254::G2Affine {x, y, infinity: bool}: 136 B, flag at byte 128 */
  MSM_AMD_G2_POINT_PREPARED = 2,   /* device-only: 128-byte records written by msm_amd_g2_bases_upload /
                                      msm_amd_g2_bases_prepare_device (opaque internal form of affine G2 points) */
  MSM_AMD_G2_POINT_TABLES = 3      /* the "points" pointer is a msm_amd_g2_tables handle */
};
enum { MSM_AMD_G2_PREPARED_BYTES = 128 };   /* record size of a prepared array */
/* Bytes per point of a HOST G2 layout; 0 for an unknown layout and for the two device-only ones. */
size_t msm_amd_g2_point_bytes(int g2_point_layout);
/* One blocking G2 MSM on the GPU, host buffers (n scalars of 32 B, n points of msm_amd_g2_point_bytes).  Unknown
 * layouts, or a null pointer with n > 0, return MSM_AMD_INPUT_ERROR.  No CPU fallback.  The window is
 * msm_amd_auto_window_size_lone(n) unless msm_amd_set_window_size forced one; msm_amd_last_timings reports the
 * stages as for one lone G1 instance (convert_ms: scalar and base conversion; accumulate_ms = accumulate_kernel_ms: the
 * accumulate kernel alone; reduce_ms: combine pass, window reduction and the copy of its partial points; total_gpu_ms:
 * the sum of the stage spans; reserved = 1; reserved2[0]: work items of the accumulate grid). */
int msm_amd_msm_g2(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars, const void* points,
                   size_t n, void* out192);
/* The same with scalars and points in device memory on ctx's device.  Also takes MSM_AMD_G2_POINT_PREPARED (d_points =
 * a prepared array) and MSM_AMD_G2_POINT_TABLES (d_points = a table handle; n must equal the table's n), which the
 * host-buffer entry points refuse with MSM_AMD_INPUT_ERROR. */
int msm_amd_msm_g2_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars,
                          const void* d_points, size_t n, void* out192);

/* The two calls above at a bounded width ("scalars of bounded width" above: bits, sign, the contract and the error of a
 * violated bound); the device form takes MSM_AMD_G2_POINT_PREPARED and MSM_AMD_G2_POINT_TABLES as well. */
int msm_amd_msm_g2_bounded(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* scalars,
                           const void* points, size_t n, uint32_t bits, int sign, void* out192);
int msm_amd_msm_g2_bounded_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout, const void* d_scalars,
                                  const void* d_points, size_t n, uint32_t bits, int sign, void* out192);

/* Persistent G2 bases (the G2 query of a Groth16 proving key is set once and multiplied by a fresh witness per proof):
 * msm_amd_bases_upload / _prepare_device / msm_amd_msm_prepared on G2.  The points (a host layout) are converted once
 * into 128-byte internal records resident on the device; free a prepared array with msm_amd_device_free.  Results are
 * byte for byte those of msm_amd_msm_g2 on the same inputs.  msm_amd_last_timings: convert_ms is then the scalar
 * conversion alone. */
int msm_amd_g2_bases_upload(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, void** d_prepared);
int msm_amd_g2_bases_prepare_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                    void* d_prepared /* n x 128 bytes */);
int msm_amd_msm_g2_prepared(msm_amd_ctx* ctx, int scalar_layout, const void* scalars /* host */, const void* d_prepared,
                            size_t n, void* out192);

/* Precomputed G2 window tables (msm_amd_tables_* on G2): 2^(c w) P_i for every window w, W x n x 128 bytes (1.9 GB for
 * 2^20 points at c = 18).  All windows share ONE set of 2^(c-1) buckets: the window reduction sums one bucket set
 * instead of W and the host Horner pass walks c bit positions instead of 254.  Built from the two host layouts;
 * window_size 0 = automatic, else 4..21 with windows * n < 2^31.  Same results byte for byte at every window.  A
 * handle belongs to its ctx and to G2: a G1 table handle here, or a G2 handle in a G1 call, is MSM_AMD_INPUT_ERROR.
 * msm_amd_destroy releases tables the caller did not free.  msm_amd_last_timings: num_windows = digit windows per
 * scalar. */
typedef struct msm_amd_g2_tables msm_amd_g2_tables;
int msm_amd_g2_tables_build(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, uint32_t window_size,
                            msm_amd_g2_tables** out);
int msm_amd_g2_tables_build_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                   uint32_t window_size, msm_amd_g2_tables** out);
int msm_amd_g2_tables_info(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, size_t* n, uint32_t* window_size,
                           uint32_t* num_windows, size_t* device_bytes);
int msm_amd_g2_tables_free(msm_amd_ctx* ctx, msm_amd_g2_tables* tables);
int msm_amd_msm_g2_tables(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, int scalar_layout,
                          const void* scalars /* host */, void* out192);
/* The CPU G2 MSM of the library (no ctx, no GPU): windowed bucket method on 4 x 64-bit limbs; threads <= 0: up to 16
 * host threads.  Same layouts and result form as msm_amd_msm_g2. */
int msm_amd_host_msm_g2(int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
                        int threads, void* out192);
/* ... at a bounded width: MSM_AMD_INPUT_ERROR, output untouched, for a record beyond the bound. */
int msm_amd_host_msm_g2_bounded(int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
                                uint32_t bits, int sign, int threads, void* out192);
/* Test aid: out[i] = start + i * step for i < n, MSM_AMD_G2_POINT_H2C_AFFINE records (host code, threads <= 0: up to
 * 16 host threads). */
int msm_amd_test_g2_progression(const void* start128, const void* step128, size_t n, int threads, void* out);
/* Raw-limb G2 test ops: operands of MSM_AMD_G2_RAW_IN_WORDS u32, results of MSM_AMD_G2_RAW_OUT_WORDS u32.
 * fq2 = 18 words (c0 limbs 0..8, c1 limbs 0..8, 29-bit internal limbs); affine = x, y (36 words);
 * XYZZ point = X, Y, ZZ, ZZZ (72 words).  Result: the fq2 or point from word 0, word 72 = 1 if the sum vanished. */
enum { MSM_AMD_G2_RAW_IN_WORDS = 72, MSM_AMD_G2_RAW_OUT_WORDS = 80 };
enum {
  MSM_AMD_G2_RAW_FQ2_MUL = 0,    /* a * b */
  MSM_AMD_G2_RAW_FQ2_SQR = 1,    /* a^2 */
  MSM_AMD_G2_RAW_PT_MADD = 2,    /* XYZZ a + affine b (madd-2008-s), neither the identity */
  MSM_AMD_G2_RAW_PT_MMADD = 3,   /* affine a + affine b, neither the identity */
  MSM_AMD_G2_RAW_PT_ADD_NZ = 4,  /* XYZZ a + XYZZ b, neither the identity (add-2008-s) */
  MSM_AMD_G2_RAW_PT_ADD = 5,     /* XYZZ a + XYZZ b, identities allowed */
  MSM_AMD_G2_RAW_PT_DOUBLE = 6,  /* 2 a, a not the identity */
  MSM_AMD_G2_RAW_FQ2_INV = 7,    /* a^-1, a != 0, a < 32 p */
  MSM_AMD_G2_RAW_PT_TO_AFFINE = 8, /* XYZZ a (not the identity) -> affine x, y in words 0..35, canonical limbs */
  /* 9 stays unknown (tests pin it as refused) */
  MSM_AMD_G2_RAW_FQ2_SQRT = 10   /* square root of the fq2 a (components normalised, < 4 p) as the G2 decompression
                                    takes it: root in words 0..17, word 72 = 1 if there is one, else all zero */
};
int msm_amd_test_op_g2(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);
/* The same bodies on the host CPU (no GPU needed). */
int msm_amd_test_op_g2_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);
/* Test aids of the G2 tables: `count` entries of window w from point `first` on, as MSM_AMD_G2_POINT_H2C_AFFINE
 * records (identity = all zero) ... */
int msm_amd_test_g2_tables_read(msm_amd_ctx* ctx, const msm_amd_g2_tables* tables, uint32_t w, size_t first,
                                size_t count, void* out);
/* ... and the host twin of the table build (no ctx, no GPU; the same bodies on the CPU): all num_windows x n entries
 * in the same form, out[(w * n + i) * 128]; points in a host layout; threads <= 0: up to 16 host threads. */
int msm_amd_test_g2_table_host(int g2_point_layout, const void* points, size_t n, uint32_t window_size,
                               uint32_t num_windows, int threads, void* out);

/* ---- point validation (G1 and G2) ------------------------------------------------------------------
 * The MSM entry points multiply whatever they are handed.  These calls judge a point array first -- the one-time check
 * of a proving key or an SRS before msm_amd_tables_build / msm_amd_g2_tables_build.  Every record gets ONE reason code,
 * the first rule that fails; the rule is the same on the GPU and in the host twins.  A key that arrives compressed goes
 * through msm_amd_decompress_points* (below) first: decompress, then check, then tables. */
enum {
  MSM_AMD_POINT_VALID = 0,           /* passes every requested check */
  MSM_AMD_POINT_NOT_REDUCED = 1,     /* some coordinate, read as a 256-bit integer in the layout's own form (the
                                        Montgomery residue), is >= p */
  MSM_AMD_POINT_NOT_ON_CURVE = 2,    /* G1: y^2 != x^3 + 3 (Jacobian layouts: Y^2 != X^3 + 3 Z^6); G2: y^2 != x^3 + 3 / (9 + u) */
  MSM_AMD_POINT_NOT_IN_SUBGROUP = 3, /* G2 only: on the curve, but [r] P != O */
  MSM_AMD_POINT_BAD_ENCODING = 4     /* compressed records only (msm_amd_decompress_points* below): flag bits that no
                                        encoder writes; never produced by the checks of this section */
};
/* Identity encodings are valid: (0, 0) / all zero in the halo2curves layouts; the infinity flag of the ark affine
 * layouts (whatever the coordinate bytes of a flagged record); Z = 0 in the two G1 Jacobian layouts (whose coordinates
 * are still range-checked). */
enum {
  MSM_AMD_CHECK_CURVE = 1,    /* rules 1 and 2 */
  MSM_AMD_CHECK_SUBGROUP = 2  /* implies CURVE and adds rule 3; on G1 (cofactor 1) accepted and equal to CURVE */
};
typedef struct msm_amd_check_report {
  uint64_t n_checked, n_invalid, n_identity;   /* n_identity: records valid as an identity encoding */
  uint64_t first_invalid;        /* smallest index with a non-zero reason; UINT64_MAX if none */
  uint32_t first_reason;         /* its reason code (0 if none) */
  uint32_t by_reason[4];         /* records per reason code (index 0 = valid) */
  float device_ms;               /* kernel time, 0 for the host twins */
} msm_amd_check_report;
/* MSM_AMD_OK means the check ran: invalid points are reported in `report`, never in the status.  n == 0: OK and an empty
 * report.  MSM_AMD_INPUT_ERROR: checks == 0 or unknown bits, a null pointer with n > 0, a null report, n >= 2^32, an
 * unknown layout or a device-only one (*_PREPARED, *_TABLES: the library's own output).  G1 takes the four host layouts,
 * G2 both of its host layouts.  reasons (n bytes, one reason code per record) may be NULL.  The ctx calls serialise on
 * the ctx and first wait -- bounded, msm_amd_set_wait_timeout_ms -- for its earlier work: a ctx that stays busy, or a
 * check that does not finish in time, returns MSM_AMD_PIPELINE_ERROR and msm_amd_last_error names the check.  Host
 * buffers go up in chunks through the ctx's page-locked staging ring. */
int msm_amd_check_points(msm_amd_ctx* ctx, int point_layout, const void* points, size_t n, uint32_t checks,
                         uint8_t* reasons, msm_amd_check_report* report);
int msm_amd_check_points_device(msm_amd_ctx* ctx, int point_layout, const void* d_points, size_t n, uint32_t checks,
                                uint8_t* d_reasons /* device memory, or NULL */, msm_amd_check_report* report);
int msm_amd_g2_check_points(msm_amd_ctx* ctx, int g2_point_layout, const void* points, size_t n, uint32_t checks,
                            uint8_t* reasons, msm_amd_check_report* report);
int msm_amd_g2_check_points_device(msm_amd_ctx* ctx, int g2_point_layout, const void* d_points, size_t n,
                                   uint32_t checks, uint8_t* d_reasons /* device memory, or NULL */,
                                   msm_amd_check_report* report);
/* The same checks on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host
 * threads. */
int msm_amd_host_check_points(int point_layout, const void* points, size_t n, uint32_t checks, int threads,
                              uint8_t* reasons, msm_amd_check_report* report);
int msm_amd_host_g2_check_points(int g2_point_layout, const void* points, size_t n, uint32_t checks, int threads,
                                 uint8_t* reasons, msm_amd_check_report* report);

/* ---- compressed points (G1 and G2) ------------------------------------------------------------------
 * Keys travel and rest compressed: x and one or two flag bits, 32 B per G1 point and 64 B per G2 point.  These calls
 * decompress on the GPU (one modular square root per G1 point; two, and an inversion, per G2 point) and compress (a few
 * instructions per point).  Both formats store x as the CANONICAL integer (not Montgomery), little-endian, 32 B; for G2
 * x.c0 comes first, then x.c1, 64 B in all.  p < 2^254, so the top two bits of the LAST byte (byte 31 for G1, byte 63
 * for G2) are free and carry the flags; "x" below is the integer after those two bits are masked off.
 *   MSM_AMD_COMPRESSED_ARK     what ark-serialize 0.4 writes for ark_bn254::G1Affine / G2Affine in compressed mode:
 *                              0x80 set: y is the LARGER of {y, p - y};  0x40 set: the record is the identity.
 *                              Order on Fq: the canonical integers.  Order on Fq2: compare c1 first, c0 on a tie.
 *   MSM_AMD_COMPRESSED_PARITY  the halo2curves-family convention:
 *                              0x80 set: the record is the identity;  0x40 set: sign(y) = 1.
 *                              G1: sign(y) is the least significant bit of canonical y.  G2: sign(y) is the least
 *                              significant bit of y.c0, or of y.c1 when y.c0 = 0 (for every y != 0 exactly one of y
 *                              and -y has sign 1).
 * The written rule is the contract.  Byte compatibility with a particular release of the crates named above is
 * UNPINNED (neither crate was available to test against) -- least certain for the G2 case of
 * PARITY.  Values from 2 on are free for further formats (gnark's big-endian form is not implemented).
 *
 * Decoding is strict.  Each record gets ONE reason code, the first rule that fails, in this order:
 *   4 MSM_AMD_POINT_BAD_ENCODING  both flag bits are set, or the identity flag is set together with any non-zero bit
 *                                 of x (a flagged identity has all other 255 / 511 bits zero)
 *   1 MSM_AMD_POINT_NOT_REDUCED   x >= p, or (G2) either component >= p
 *   2 MSM_AMD_POINT_NOT_ON_CURVE  x^3 + 3 (G1) or x^3 + 3 / (9 + u) (G2) has no square root
 *   0 MSM_AMD_POINT_VALID         otherwise.  Reason 3 is never produced here: the subgroup test stays with
 *                                 msm_amd_g2_check_points*.  Recipe for an untrusted G2 key: decompress, then
 *                                 msm_amd_g2_check_points_device(..., MSM_AMD_CHECK_SUBGROUP) on the output, then
 *                                 msm_amd_g2_tables_build_device. */
enum {
  MSM_AMD_COMPRESSED_ARK = 0,
  MSM_AMD_COMPRESSED_PARITY = 1
};
typedef struct msm_amd_decompress_report {
  uint64_t n_checked, n_invalid, n_identity, first_invalid;  /* as msm_amd_check_report */
  uint32_t first_reason, by_reason[5];
  float device_ms;
} msm_amd_decompress_report;
/* Bytes per compressed record: 32 for group 1, 64 for group 2; 0 for an unknown format or group. */
size_t msm_amd_compressed_bytes(int format, int group /* 1 or 2 */);
/* Decompression: n records of `in` -> n records of `out` in point_layout_out, reasons (n bytes, may be NULL) and the
 * report.  Output layouts: G1 MSM_AMD_POINT_H2C_AFFINE / _ARK_AFFINE, G2 MSM_AMD_G2_POINT_H2C_AFFINE / _ARK_AFFINE; the
 * _device calls also take MSM_AMD_POINT_PREPARED / MSM_AMD_G2_POINT_PREPARED and then write, bit for bit, the 64-byte /
 * 128-byte records msm_amd_bases_prepare_device / msm_amd_g2_bases_prepare_device would write from the decompressed
 * affine points: a compressed key on the device becomes MSM-ready bases in one pass, usable at once with
 * msm_amd_msm_device / msm_amd_msm_g2_device / *_tables_build_device.  An invalid record yields the layout's identity
 * encoding in `out` (all zero; ark affine: zero coordinates and the flag byte 1) and its reason in `reasons`: the output
 * is always fully defined.
 * Status and arguments as msm_amd_check_points*: MSM_AMD_OK means the pass ran; n == 0: OK and an empty report;
 * MSM_AMD_INPUT_ERROR: an unknown format or layout, *_TABLES, *_PREPARED on a host-buffer or host-twin call, a null
 * pointer with n > 0, a null report, n >= 2^32.  The ctx calls serialise on the ctx and first wait -- bounded -- for its
 * earlier work (a busy ctx: MSM_AMD_PIPELINE_ERROR, msm_amd_last_error names the call); host buffers go up in chunks
 * through the page-locked staging ring; a G2 call touches the G2 state of the ctx only. */
int msm_amd_decompress_points(msm_amd_ctx* ctx, int format, const void* in, size_t n, int point_layout_out, void* out,
                              uint8_t* reasons, msm_amd_decompress_report* report);
int msm_amd_decompress_points_device(msm_amd_ctx* ctx, int format, const void* d_in, size_t n, int point_layout_out,
                                     void* d_out, uint8_t* d_reasons, msm_amd_decompress_report* report);
int msm_amd_g2_decompress_points(msm_amd_ctx* ctx, int format, const void* in, size_t n, int g2_point_layout_out,
                                 void* out, uint8_t* reasons, msm_amd_decompress_report* report);
int msm_amd_g2_decompress_points_device(msm_amd_ctx* ctx, int format, const void* d_in, size_t n,
                                        int g2_point_layout_out, void* d_out, uint8_t* d_reasons,
                                        msm_amd_decompress_report* report);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads. */
int msm_amd_host_decompress_points(int format, const void* in, size_t n, int point_layout_out, int threads, void* out,
                                   uint8_t* reasons, msm_amd_decompress_report* report);
int msm_amd_host_g2_decompress_points(int format, const void* in, size_t n, int g2_point_layout_out, int threads,
                                      void* out, uint8_t* reasons, msm_amd_decompress_report* report);
/* Compression: n affine records (the two affine host layouts of the group) -> n compressed records.  An identity
 * encoding becomes the format's identity record.  A record whose stored coordinate is >= p is written as all 0xFF (no
 * valid encoding in either format) and counted in *n_bad (may be NULL).  Points are not checked for being on the curve.
 * Status and argument rules as above (no report; *_PREPARED and *_TABLES are refused everywhere). */
int msm_amd_compress_points(msm_amd_ctx* ctx, int point_layout_in, const void* in, size_t n, int format, void* out,
                            uint64_t* n_bad);
int msm_amd_compress_points_device(msm_amd_ctx* ctx, int point_layout_in, const void* d_in, size_t n, int format,
                                   void* d_out, uint64_t* n_bad);
int msm_amd_g2_compress_points(msm_amd_ctx* ctx, int g2_point_layout_in, const void* in, size_t n, int format, void* out,
                               uint64_t* n_bad);
int msm_amd_g2_compress_points_device(msm_amd_ctx* ctx, int g2_point_layout_in, const void* d_in, size_t n, int format,
                                      void* d_out, uint64_t* n_bad);
int msm_amd_host_compress_points(int point_layout_in, const void* in, size_t n, int format, int threads, void* out,
                                 uint64_t* n_bad);
int msm_amd_host_g2_compress_points(int g2_point_layout_in, const void* in, size_t n, int format, int threads, void* out,
                                    uint64_t* n_bad);

/* ---- batch scalar multiplication (G1 and G2) ---------------------------------------------------------
 * Every call above CONSUMES a point array; these produce one: out[i] = [s_i] P_i (MSM_AMD_MUL_BASE_EACH) or
 * out[i] = [s_i] P for one base P (MSM_AMD_MUL_BASE_ONE; arkworks' FixedBase::msm / batch_mul) -- an SRS or a test key
 * ([tau^i] G), a ceremony contribution (P_i -> [tau^i] P_i), a re-randomised key, benchmark inputs.
 * Scalars: n records of 32 B in one of the MSM_AMD_SCALAR_* layouts, read exactly as the MSM entry points read them (a
 * canonical layout is reduced mod r).  The result is the group element [s] P for that integer s < r, written as its
 * CANONICAL affine coordinates, so the bytes are unique; it is multiplied as a curve point whatever its order (a G2 base
 * outside the r-torsion included).
 * points: n records (BASE_EACH) or ONE record (BASE_ONE) of point_layout_in -- G1: the four host layouts, G2: both host
 * layouts; the _device calls also take MSM_AMD_POINT_PREPARED / MSM_AMD_G2_POINT_PREPARED (BASE_ONE: one prepared record).
 * out: n records of point_layout_out, one of the two affine host layouts of the group; the _device calls also take
 * *_PREPARED and then write, bit for bit, the records msm_amd_bases_prepare_device / msm_amd_g2_bases_prepare_device would
 * write from the affine result: a generated array is MSM-ready at once (msm_amd_msm_device, *_tables_build_device,
 * *_check_points_device, *_compress_points_device take it as it is).  A result that is the identity (s = 0, an identity
 * base, [s] P = O for a G2 base of small order) is written as the layout's identity encoding, exactly as the decompress
 * calls write it; the output is always fully defined.  Inputs are NOT validated: a base that is not on the curve gives
 * unspecified but defined bytes.
 * BASE_ONE always runs the fixed-base path (a table of [d 2^(8 w)] P, at most 32 mixed additions per output), BASE_EACH
 * a 256-step double-and-add ladder per record; both end in a batched normalisation, one inversion per 16 consecutive
 * outputs.  The call may run in chunks of outputs (one intermediate record per output of a chunk); no byte of the
 * result depends on that.
 * Status and arguments as msm_amd_check_points*: n == 0: MSM_AMD_OK, nothing is touched; MSM_AMD_INPUT_ERROR: an unknown
 * layout or base mode, *_TABLES, *_PREPARED on a host-buffer call or a host twin, a null pointer with n > 0, n >= 2^32.
 * The ctx calls serialise on the ctx and first wait -- bounded -- for its earlier work (a busy ctx:
 * MSM_AMD_PIPELINE_ERROR, msm_amd_last_error names the call); host buffers go up through the page-locked staging ring;
 * a G2 call touches the G2 state of the ctx only. */
enum {
  MSM_AMD_MUL_BASE_EACH = 0,  /* points: n records, out[i] = [s_i] P_i */
  MSM_AMD_MUL_BASE_ONE = 1    /* points: ONE record, out[i] = [s_i] P */
};
int msm_amd_mul_points(msm_amd_ctx* ctx, int scalar_layout, int point_layout_in, int base_mode, const void* scalars,
                       const void* points, size_t n, int point_layout_out, void* out);
int msm_amd_mul_points_device(msm_amd_ctx* ctx, int scalar_layout, int point_layout_in, int base_mode,
                              const void* d_scalars, const void* d_points, size_t n, int point_layout_out, void* d_out);
int msm_amd_g2_mul_points(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout_in, int base_mode, const void* scalars,
                          const void* points, size_t n, int g2_point_layout_out, void* out);
int msm_amd_g2_mul_points_device(msm_amd_ctx* ctx, int scalar_layout, int g2_point_layout_in, int base_mode,
                                 const void* d_scalars, const void* d_points, size_t n, int g2_point_layout_out,
                                 void* d_out);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads. */
int msm_amd_host_mul_points(int scalar_layout, int point_layout_in, int base_mode, const void* scalars, const void* points,
                            size_t n, int point_layout_out, int threads, void* out);
int msm_amd_host_g2_mul_points(int scalar_layout, int g2_point_layout_in, int base_mode, const void* scalars,
                               const void* points, size_t n, int g2_point_layout_out, int threads, void* out);
/* Test aid (no ctx): the constants of the two paths for group 1 or 2 -- out[0] window c of the fixed-base table,
 * [1] its windows W, [2] its entries W 2^(c-1), [3] K, the number of consecutive outputs that share one inversion.
 * (Development knob MSM_AMD_MUL_CHUNK at msm_amd_init: outputs per chunk of the ctx calls, rounded up to a multiple
 * of K; default 2^18.) */
int msm_amd_test_mul_plan(int group /* 1 or 2 */, uint32_t out[4]);
/* Test aid: one stage of msm_amd_mul_points on input the caller wrote, on the GPU (host buffers, staged like the host-buffer
 * calls) and on the CPU (the same bodies compiled for the host).  group: 1 or 2.
 *   MSM_AMD_MUL_STAGE_FIXED      the signed-digit walk of BASE_ONE over the caller's table.  in: n scalars of 32 bytes,
 *     layout: their MSM_AMD_SCALAR_* layout; table: entries [2] of msm_amd_test_mul_plan, entry w 2^(c-1) + d - 1 standing
 *     for [d 2^(c w)] P, each the canonical x, y of the internal Montgomery domain (radix 2^261; G2: x.c0, x.c1, y.c0,
 *     y.c1), 32 little-endian bytes per coordinate; an entry whose first coordinate is 2^256 - 1 is the identity.
 *     out: n raw XYZZ records as the walk leaves them, 36 (G1) / 72 (G2) words of 29-bit limbs: X, Y, ZZ, ZZZ, G2 c0
 *     before c1; ZZ limbs all zero = identity.
 *   MSM_AMD_MUL_STAGE_NORMALISE  the shared inversion.  in: n such XYZZ records inside the point invariant (X < 10 p,
 *     Y < 6 p, ZZ < 2.8 p, ZZZ < 2 p; G2: 1.21, 13.4, 3.2, 2.04 per component; limbs 0..7 <= 2^29 + 7), layout: an affine
 *     host point layout of the group; table is not read.  out: n affine records of that layout, consecutive groups of
 *     [3] of msm_amd_test_mul_plan sharing one inversion.  The stage runs on a copy: `in` is not written.
 *   MSM_AMD_MUL_STAGE_NORMALISE_RECORDS  the same stage on the same input; out: that copy as the stage leaves it, n XYZZ
 *     records holding the intermediates of the shared inversion in the places of X, Y, ZZ, ZZZ: X ZZZ, ZZ Y,
 *     a_i = ZZ ZZZ and the prefix product before record i (an identity record: exact zero limbs, zero limbs, one, the
 *     prefix).  For the bound checks of the chain; the affine bytes are dropped.
 * MSM_AMD_INPUT_ERROR for an unknown group, stage or layout and for n >= 2^32; n == 0 touches nothing; a null pointer
 * with n > 0 is refused. */
enum { MSM_AMD_MUL_STAGE_FIXED = 0, MSM_AMD_MUL_STAGE_NORMALISE = 1, MSM_AMD_MUL_STAGE_NORMALISE_RECORDS = 2 };
int msm_amd_test_mul_stage(msm_amd_ctx* ctx, int group, int which, int layout, const void* in, const void* table,
                           size_t n, void* out);
int msm_amd_test_mul_stage_host(int group, int which, int layout, const void* in, const void* table, size_t n, void* out);

/* ---- number-theoretic transform over Fr ----------------------------------------------------------------
 * The MSM calls CONSUME device-resident scalars; in a prover those scalars are outputs of a transform over Fr (halo2's
 * best_fft next to best_multiexp, the inverse and coset transforms of Groth16's h-query).  These calls produce them
 * where the MSM reads them: msm_amd_ntt_device(..., MSM_AMD_NTT_INVERSE, ...) and msm_amd_msm_device on the same pointer.
 * Lengths: r - 1 = 2^28 t with t odd, so n = 2^log_n, 0 <= log_n <= 28, and the primitive n-th root is
 * w = rho^(2^(28 - log_n)) for a 2^28-th root rho chosen by an enum, because the two crate families differ:
 *   MSM_AMD_NTT_ROOT_ARK  rho = 5^t mod r = 19103219067921713944291392827692070036145651957329286315305642004821462161904
 *   MSM_AMD_NTT_ROOT_H2C  rho = 7^t mod r = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
 * The library derives rho as g^t on the host; tests/test_ntt_host.py holds the two values and checks rho^(2^27) = -1.
 * UNPINNED: that they equal ark-bn254's TWO_ADIC_ROOT_OF_UNITY and halo2curves' ROOT_OF_UNITY is recollection only
 * (neither crate was available to test against).
 * Definitions, all mod r, natural order in and out; g is an optional coset shift (shift32; NULL: g = 1):
 *   MSM_AMD_NTT_FORWARD  out[k] = sum_{i<n} in[i] g^i w^(i k): the evaluations of the polynomial on g H
 *   MSM_AMD_NTT_INVERSE  out[i] = g^-i n^-1 sum_{k<n} in[k] w^(-i k): the exact inverse of FORWARD with the same g (the
 *                        library inverts g and n on the host)
 * Scalars: 32-byte records in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE (MSM_AMD_SCALAR_CANON_BE32:
 * MSM_AMD_INPUT_ERROR); the shift and the output use the layout of the input.  Inputs are read as the MSM reads them:
 * any 256-bit value is taken mod r.  Every output is the fully reduced residue, so the bytes are unique.
 * A call transforms n_vec >= 1 vectors stored back to back, n_vec n < 2^32.
 * A domain holds the twiddles of one (root, log_n) on the ctx's device -- w^j for j < n/2, device_bytes = 16 n (32 for
 * n = 1) -- and serves both directions.  msm_amd_destroy releases the domains the caller did not free.
 * Status: n_vec == 0: MSM_AMD_OK, nothing is touched.  MSM_AMD_INPUT_ERROR: an unknown root, direction or layout;
 * log_n > 28; a null pointer with n_vec > 0; g = 0 mod r; n_vec n >= 2^32; a domain handle of another ctx, a freed one or
 * a table handle; device buffers that are not 16-byte aligned or that overlap without being equal -- d_out == d_in (in
 * place) and disjoint buffers are both valid, and an out-of-place call leaves d_in unchanged.
 * The ctx calls serialise on the ctx and first wait -- bounded -- for its earlier work (a busy ctx:
 * MSM_AMD_PIPELINE_ERROR, msm_amd_last_error names the call); a transform of more than 2^10 elements uses one
 * ctx-owned buffer of the size of the batch; msm_amd_ntt uploads the batch through the page-locked staging ring.
 * (Development knob MSM_AMD_NTT_TILE_LOG = 2 .. 10 at msm_amd_init: elements per workgroup of a pass as a power of two;
 * default 10.  No byte of a result depends on it.) */
enum { MSM_AMD_NTT_ROOT_ARK = 0, MSM_AMD_NTT_ROOT_H2C = 1 };
enum { MSM_AMD_NTT_FORWARD = 0, MSM_AMD_NTT_INVERSE = 1 };
typedef struct msm_amd_ntt_domain msm_amd_ntt_domain;
int msm_amd_ntt_domain_build(msm_amd_ctx* ctx, int root, uint32_t log_n, msm_amd_ntt_domain** out);
int msm_amd_ntt_domain_info(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int* root, uint32_t* log_n,
                            size_t* device_bytes, void* omega32 /* w, 32 B MONT_LE; may be NULL, like the others */);
int msm_amd_ntt_domain_free(msm_amd_ctx* ctx, msm_amd_ntt_domain* domain);
int msm_amd_ntt(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout,
                const void* shift32 /* g in scalar_layout, or NULL */, const void* in, void* out, size_t n_vec);
/* kernel_ms (optional, as msm_amd_sort_pairs_device): device time of the passes between two events */
int msm_amd_ntt_device(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout,
                       const void* shift32 /* HOST memory, or NULL */, const void* d_in, void* d_out, size_t n_vec,
                       float* kernel_ms);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads. */
int msm_amd_host_ntt(int root, uint32_t log_n, int direction, int scalar_layout, const void* shift32, const void* in,
                     void* out, size_t n_vec, int threads);
/* Test aids of the transform.  A call of log_n levels at a tile of 2^tile_log elements per workgroup (2 .. 10; the ctx
 * calls use MSM_AMD_NTT_TILE_LOG) runs ceil(log_n / tile_log) passes (one for log_n = 0); pass k covers the levels
 * level0 .. level0 + levels - 1 of the decimation-in-frequency network, on tiles of 2^levels elements at stride
 * 2^sigma, and a workgroup holds 2^low neighbouring index bits below the tile bits.
 * msm_amd_test_ntt_plan (no ctx): out[0] = the pass count, then level0, levels, sigma, low of every pass -- out holds
 *   1 + 4 * 28 words.  The values are the ones the kernel launches compute.
 * msm_amd_test_ntt_slots (no ctx): out[m], m < 2^tile_log = the flat element index v n + i (over a batch of any size:
 *   the kernel drops indices >= n_vec n) that slot m of workgroup wg < 2^32 holds in pass `pass` of that plan; the
 *   function the kernel calls, compiled for the host.
 * msm_amd_test_ntt_passes: msm_amd_ntt stopped after the first `passes` passes of its plan, 1 <= passes <= the pass
 *   count.  Below the count, out = the ctx's pass buffer as those passes left it: n_vec n fully reduced Montgomery
 *   residues (whatever scalar_layout) at the positions of the network -- what msm_amd_test_host_ntt_levels writes for
 *   the levels those passes cover.  With the full count, out = what msm_amd_ntt returns.
 * msm_amd_test_host_ntt_levels (no ctx): msm_amd_host_ntt stopped after `levels` <= log_n levels; out = its work array
 *   as it stands: Montgomery residues, input conversion and the FORWARD shift applied, no permutation to natural
 *   order, no INVERSE scaling (levels = log_n: position bitrev(k) holds the k-th sum).
 * msm_amd_test_ntt_twiddles: `count` records of the domain's table from entry `first`: out[j] = w^(first + j), MONT_LE,
 *   first + count <= n / 2.
 * MSM_AMD_INPUT_ERROR for values outside these ranges and what msm_amd_ntt / msm_amd_host_ntt refuse; a null pointer with
 * work to do is refused; n_vec == 0 or count == 0 touches nothing. */
int msm_amd_test_ntt_plan(uint32_t log_n, uint32_t tile_log, uint32_t* out);
int msm_amd_test_ntt_slots(uint32_t log_n, uint32_t tile_log, uint32_t pass, uint64_t wg, uint64_t* out);
int msm_amd_test_ntt_passes(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int scalar_layout,
                            const void* shift32, const void* in, void* out, size_t n_vec, uint32_t passes);
int msm_amd_test_host_ntt_levels(int root, uint32_t log_n, int direction, int scalar_layout, const void* shift32,
                                 const void* in, void* out, size_t n_vec, uint32_t levels, int threads);
int msm_amd_test_ntt_twiddles(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, size_t first, size_t count, void* out);

/* ---- transform over G1 points: a monomial SRS to a Lagrange SRS ------------------------------------------
 * A KZG prover that commits to columns in evaluation form (halo2, PLONK) needs the Lagrange SRS [L_i(tau)] G.  Nobody
 * knows tau, so it can only be made by running the inverse transform over the group elements [tau^j] G of the monomial
 * SRS (halo2's g_to_lagrange; UNPINNED: that halo2 uses exactly w^-1 and n^-1 is recollection only, like the roots
 * above).  These calls do that with the domain handles of the scalar transform.
 * Definitions, natural order in and out, additions in G1, w the domain's root, n = 2^log_n:
 *   MSM_AMD_NTT_FORWARD  out[k] = sum_{i<n} [w^(i k)] in[i]
 *   MSM_AMD_NTT_INVERSE  out[i] = [n^-1] sum_{k<n} [w^(-i k)] in[k]: the exact inverse of FORWARD.  With
 *                        MSM_AMD_NTT_ROOT_H2C on in[j] = [tau^j] G it yields [L_i(tau)] G.
 * Limits: one vector per call, no coset shift, G1 only.
 * Points.  Input: the four G1 host layouts; the _device call also takes MSM_AMD_POINT_PREPARED.  Output: the two affine
 * host layouts; the _device call also takes MSM_AMD_POINT_PREPARED and then writes the bytes msm_amd_bases_prepare_device
 * would write from the affine result, so msm_amd_msm_device, msm_amd_tables_build_device, msm_amd_check_points_device and
 * msm_amd_compress_points_device take the output as it is.  The output is canonical affine, so the bytes are unique; an
 * identity result is the layout's identity encoding, as msm_amd_mul_points writes it.  Identity inputs are ordinary
 * operands.  Inputs are not validated: an off-curve input gives unspecified but defined bytes.
 * Buffers of the _device call: d_out == d_in (in place; the first pass consumes the input into ctx-owned work buffers
 * before anything is written) and disjoint buffers are both valid, and an out-of-place call leaves d_in unchanged;
 * buffers that overlap without being equal are refused.  The ctx owns two work arrays of 64 n bytes each.
 * Status, as msm_amd_ntt and msm_amd_mul_points.  MSM_AMD_INPUT_ERROR: a null pointer; a domain handle of another ctx, a
 * freed one or a table handle; an unknown direction or layout; MSM_AMD_POINT_TABLES; MSM_AMD_POINT_PREPARED on a
 * host-buffer call or on the twin; overlapping device buffers; the twin: an unknown root, log_n > 28.  The ctx calls
 * serialise on the ctx and first wait -- bounded -- for its earlier work (a busy ctx: MSM_AMD_PIPELINE_ERROR,
 * msm_amd_last_error names the call); every buffer is sized on the idle ctx before anything is enqueued.  log_n = 0
 * copies the one record through the normalisation.  (MSM_AMD_MUL_CHUNK also sets the outputs per chunk of a level; no
 * byte of a result depends on it.) */
int msm_amd_ntt_points(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                       const void* in, int point_layout_out, void* out);
/* kernel_ms (optional): device time of all passes between two events */
int msm_amd_ntt_points_device(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                              const void* d_in, int point_layout_out, void* d_out, float* kernel_ms);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads, and
 * never more than 16. */
int msm_amd_host_ntt_points(int root, uint32_t log_n, int direction, int point_layout_in, const void* in,
                            int point_layout_out, void* out, int threads);
/* Test aids (host buffers): the call stopped after `levels` <= log_n levels of its network; out = the work array as
 * affine records of point_layout_out in network order, no final scaling.  The network is decimation in time:
 *   load:  work[bitrev(j)] = in[j]
 *   level l = 1 .. log_n, for every block base b that is a multiple of 2^l and every i < 2^(l-1):
 *     u = work[b + i],  v = [w^(+-i n / 2^l)] work[b + i + 2^(l-1)]      (- for INVERSE)
 *     work[b + i] = u + v,  work[b + i + 2^(l-1)] = u - v
 * so levels = log_n with FORWARD equals the public call, and levels = 0 is the bit-reversed input.
 * levels > log_n: MSM_AMD_INPUT_ERROR; the rest as the calls they stop. */
int msm_amd_test_ntt_points_levels(msm_amd_ctx* ctx, const msm_amd_ntt_domain* domain, int direction, int point_layout_in,
                                   const void* in, uint32_t levels, int point_layout_out, void* out);
int msm_amd_test_host_ntt_points_levels(int root, uint32_t log_n, int direction, int point_layout_in, const void* in,
                                        uint32_t levels, int point_layout_out, void* out, int threads);

/* ---- vectors over Fr: element-wise ops, batch inversion, prefix products ----------------------------------
 * Between a transform and an MSM a prover does arithmetic on whole vectors of Fr: Groth16's h = (a.b - c) (g^n - 1)^-1
 * between the coset transforms, the grand products z[i+1] = z[i] num[i] / den[i] of the halo2 / PLONK permutation and
 * lookup arguments (arkworks batch_inversion, halo2 batch_invert, then a running product), random linear combinations
 * a + k b before a commitment.  These calls do it where the transform leaves the data and the MSM reads it.
 * Scalars as in msm_amd_ntt*: 32-byte records in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE
 * (MSM_AMD_SCALAR_CANON_BE32: MSM_AMD_INPUT_ERROR); any 256-bit input is taken mod r; every output is the fully reduced
 * residue in the layout of the input, so the bytes are unique.  k32 is one record in the same layout, in HOST memory for
 * every call.
 * Aliasing: out may be any operand itself (in place); operands may alias each other freely (a == b squares); an
 * out-of-place call leaves its inputs unchanged.
 * Sizes: n == 0 (or n_vec == 0): MSM_AMD_OK, nothing is touched, *n_zero = 0.  MSM_AMD_INPUT_ERROR: n >= 2^32 (prefix
 * products: n n_vec >= 2^32); an unknown op, mode or layout; a null pointer for an operand the op reads (operands the
 * op does not read, and k32 for ops without k, are ignored); device pointers that are not 16-byte aligned; an output
 * that overlaps an operand without being equal to it.
 * The ctx calls serialise on the ctx and first wait -- bounded -- for its earlier work (a busy ctx:
 * MSM_AMD_PIPELINE_ERROR, msm_amd_last_error names the call).  The host-buffer forms upload through the page-locked
 * staging ring into ctx-owned buffers.  kernel_ms (optional): device time of the kernels between events.
 * msm_amd_fr_batch_inverse*: ONE field inversion per call.  The device multiplies the records up (zeros read as one),
 * T -- the product of everything non-zero -- and the zero count come back in one 64-byte copy, the host inverts T, and
 * a last kernel turns T^-1 into every record's inverse: two bounded waits per call, kernel_ms is the sum of the two
 * device spans.  All records zero: T = 1, every output 0, *n_zero = n.
 * msm_amd_fr_prefix_product*: a multi-launch scan in stream order (tile products, the scan of the tile products --
 * recursively past 2^18 records per vector -- then the tiles); it uses ctx-owned memory of about n n_vec / 2^9 records.
 * (Development knob MSM_AMD_FR_TILE_LOG = 2 .. 9 at msm_amd_init: records per tile as a power of two; default 9, the
 * inversion uses at most 8.  No byte of a result depends on it.) */
enum { MSM_AMD_FR_ADD = 0,           /* out = a + b            */
       MSM_AMD_FR_SUB = 1,           /* out = a - b            */
       MSM_AMD_FR_MUL = 2,           /* out = a b              */
       MSM_AMD_FR_SCALE = 3,         /* out = k a              */
       MSM_AMD_FR_AXPY = 4,          /* out = a + k b          */
       MSM_AMD_FR_MULSUB_SCALE = 5   /* out = k (a b - c)      */ };
int msm_amd_fr_map(msm_amd_ctx* ctx, int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c,
                   size_t n, void* out);
int msm_amd_fr_map_device(msm_amd_ctx* ctx, int op, int scalar_layout, const void* k32 /* HOST memory */, const void* d_a,
                          const void* d_b, const void* d_c, size_t n, void* d_out, float* kernel_ms);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads. */
int msm_amd_host_fr_map(int op, int scalar_layout, const void* k32, const void* a, const void* b, const void* c, size_t n,
                        int threads, void* out);

/* out[i] = in[i]^-1; in[i] = 0 mod r gives out[i] = 0 (arkworks batch_inversion / halo2 batch_invert), counted in
 * *n_zero (optional) */
int msm_amd_fr_batch_inverse(msm_amd_ctx* ctx, int scalar_layout, const void* in, size_t n, void* out, uint64_t* n_zero);
int msm_amd_fr_batch_inverse_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_in, size_t n, void* d_out,
                                    uint64_t* n_zero, float* kernel_ms);
int msm_amd_host_fr_batch_inverse(int scalar_layout, const void* in, size_t n, int threads, void* out, uint64_t* n_zero);

enum { MSM_AMD_FR_PREFIX_INCLUSIVE = 0,  /* out[i] = prod_{j<=i} in[j]             */
       MSM_AMD_FR_PREFIX_EXCLUSIVE = 1   /* out[0] = 1, out[i] = prod_{j<i} in[j]  */ };
/* n_vec vectors of n records back to back, any n >= 1 (not only powers of two); the product restarts at every vector */
int msm_amd_fr_prefix_product(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec,
                              void* out);
int msm_amd_fr_prefix_product_device(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* d_in, size_t n, size_t n_vec,
                                     void* d_out, float* kernel_ms);
int msm_amd_host_fr_prefix_product(int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, int threads,
                                   void* out);
/* The running sums on the same scan plan, workspace, modes, sizes, aliasing rules and knob: out[i] = sum_{j<=i} in[j]
 * (INCLUSIVE) or out[0] = 0, out[i] = sum_{j<i} in[j] (EXCLUSIVE), restarting at every vector: logUp's
 * phi[i+1] = phi[i] + h_f[i] - h_t[i]. */
int msm_amd_fr_prefix_sum(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, void* out);
int msm_amd_fr_prefix_sum_device(msm_amd_ctx* ctx, int scalar_layout, int mode, const void* d_in, size_t n, size_t n_vec,
                                 void* d_out, float* kernel_ms);
int msm_amd_host_fr_prefix_sum(int scalar_layout, int mode, const void* in, size_t n, size_t n_vec, int threads, void* out);

/* out[i] = a[i] + k: beta + f[i] of a log-derivative lookup, the + gamma of PLONK's f + beta sigma + gamma (and, over a
 * buffer of zeros, a fill).  An entry point of its own: msm_amd_fr_map has no seventh op.  Sizes, aliasing (out == a or
 * disjoint) and errors as for msm_amd_fr_map with one operand; k32 is required. */
int msm_amd_fr_shift(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* a, size_t n, void* out);
int msm_amd_fr_shift_device(msm_amd_ctx* ctx, int scalar_layout, const void* k32 /* HOST memory */, const void* d_a, size_t n,
                            void* d_out, float* kernel_ms);
int msm_amd_host_fr_shift(int scalar_layout, const void* k32, const void* a, size_t n, int threads, void* out);

/* ---- polynomials over Fr: evaluate, divide by X - z, combine ----------------------------------------------
 * What a KZG opening does between the transforms and the MSM of the quotient (halo2 eval_polynomial and kate_division,
 * arkworks DensePolynomial / (X - z); the fold f = sum_v k^v p_v of a GWC / SHPLONK multi-opening).  A polynomial is n
 * coefficients, lowest degree first; n_vec polynomials lie back to back.  Records, layouts, reduction of any 256-bit
 * word, alignment, n n_vec < 2^32 with any n >= 1, the empty calls (n == 0 or n_vec == 0: MSM_AMD_OK, nothing is
 * touched), the bounded waits and msm_amd_last_error are those of msm_amd_fr_prefix_product*.  z32 / k32 is one record
 * in the same layout, in HOST memory for every call; y_out / rem_out are n_vec records in HOST memory for every call
 * (they come back in one copy through ctx-owned page-locked memory, in the call's one bounded wait), fully reduced.
 * The device side runs on the tiles and levels of the prefix products (ctx-owned memory of about n n_vec / 2^9
 * records plus n_vec): tiles start at index 0 of a polynomial, level k + 1 holds the values of the tiles of level k
 * and is the same problem at the point z^(2^T); the host squares z about 40 times per call and every kernel gets the
 * powers it needs by value. */
/* y[v] = sum_i c_v[i] z^i.  y_out null with work to do: MSM_AMD_INPUT_ERROR. */
int msm_amd_fr_poly_eval(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* coeffs, size_t n, size_t n_vec,
                         void* y_out);
int msm_amd_fr_poly_eval_device(msm_amd_ctx* ctx, int scalar_layout, const void* z32 /* HOST memory */, const void* d_coeffs,
                                size_t n, size_t n_vec, void* y_out /* HOST memory */, float* kernel_ms);
int msm_amd_host_fr_poly_eval(int scalar_layout, const void* z32, const void* coeffs, size_t n, size_t n_vec, int threads,
                              void* y_out);
/* With s_i = sum_{j >= i} c_j z^(j - i):  out[i] = s_(i+1) for i < n - 1 and out[n - 1] = 0 -- the n - 1 coefficients of
 * (p(X) - p(z)) / (X - z), padded to n so that the MSM of the quotient takes the same n bases --, rem[v] = s_0 = p_v(z)
 * (rem_out may be null).  out == in (in place) or disjoint: an out-of-place call leaves `in` unchanged, a partial
 * overlap is MSM_AMD_INPUT_ERROR. */
int msm_amd_fr_poly_div_linear(msm_amd_ctx* ctx, int scalar_layout, const void* z32, const void* in, size_t n, size_t n_vec,
                               void* out, void* rem_out);
int msm_amd_fr_poly_div_linear_device(msm_amd_ctx* ctx, int scalar_layout, const void* z32 /* HOST memory */,
                                      const void* d_in, size_t n, size_t n_vec, void* d_out, void* rem_out /* HOST memory */,
                                      float* kernel_ms);
int msm_amd_host_fr_poly_div_linear(int scalar_layout, const void* z32, const void* in, size_t n, size_t n_vec, int threads,
                                    void* out, void* rem_out);
/* out[i] = sum_{v < n_vec} k^v a[v n + i], i < n: n records.  out may be the first vector of a (out == a) or disjoint
 * from all n n_vec records of a; anything else is MSM_AMD_INPUT_ERROR. */
int msm_amd_fr_lincomb(msm_amd_ctx* ctx, int scalar_layout, const void* k32, const void* a, size_t n, size_t n_vec, void* out);
int msm_amd_fr_lincomb_device(msm_amd_ctx* ctx, int scalar_layout, const void* k32 /* HOST memory */, const void* d_a, size_t n,
                              size_t n_vec, void* d_out, float* kernel_ms);
int msm_amd_host_fr_lincomb(int scalar_layout, const void* k32, const void* a, size_t n, size_t n_vec, int threads, void* out);

/* Several points in one pass: the multi-point opening at the end of a halo2 / PLONK proof -- every column at all of its
 * rotations (z, w z, w^-1 z, ..), and SHPLONK's division of a rotation set's folded polynomial by the set's vanishing
 * polynomial Z_S(X) = prod_j (X - z_j), which upstream does as div_by_vanishing: k chained kate_divisions.  z is k records
 * in HOST memory, 1 <= k <= MSM_AMD_POLY_MAX_POINTS, in scalar_layout, any 256-bit word taken mod r.  mem
 * (MSM_AMD_MEM_HOST / MSM_AMD_MEM_DEVICE, below) says where coeffs / in / out lie, as for msm_amd_fr_sort; y_out / vals_out
 * are HOST memory either way and come back through ctx-owned page-locked memory in the call's one bounded wait.  Records,
 * layouts, alignment of device pointers, n n_vec < 2^32 with any n >= 1, the empty calls and msm_amd_last_error are
 * those of msm_amd_fr_poly_*.  The launches are those of ONE point whatever k is (levels for the evaluation, 2 levels - 1
 * for the division): level 0 reads every tile once and carries k scans through it, the upper levels hold k copies of the
 * single-point totals (ctx-owned memory of about k n n_vec / 2^9 records plus k n_vec).  The division uses
 *     q_i = sum_j w_j s^(j)_(i+1),   w_j = 1 / prod_(m != j) (z_j - z_m),   s^(j)_i = sum_(t >= i) c_t z_j^(t - i);
 * the host inverts once per call for the k weights.  DESIGN.md section 8.18.
 * MSM_AMD_INPUT_ERROR, with the reason in msm_amd_last_error and no byte of out, y_out or vals_out written: k == 0 or
 * k > MSM_AMD_POLY_MAX_POINTS, an unknown mem or layout, a null z, a null required pointer with work to do, a partial
 * overlap of out and in and, for the division only, two points that are equal mod r (the raw words 1 and r + 1, say): the
 * message names both indices.  k == 1 gives the bytes of msm_amd_fr_poly_eval* / msm_amd_fr_poly_div_linear*. */
enum { MSM_AMD_POLY_MAX_POINTS = 8 };
/* y[v k + j] = p_v(z_j): n_vec k HOST records, fully reduced.  Points may repeat. */
int msm_amd_fr_poly_eval_points(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* z /* k HOST records */, size_t k,
                                const void* coeffs, size_t n, size_t n_vec, void* y_out /* HOST memory */, float* kernel_ms);
/* out = the floor quotient p_v div prod_j (X - z_j), n records per polynomial of which the top min(k, n) are zero -- the
 * coefficients of upstream's div_by_vanishing(p_v, [z_0 .. z_(k-1)]), the same whether or not the caller subtracted the
 * remainder r(X) first; n < k is a valid call and leaves zeros.  In place (out == in) or disjoint: an out-of-place call
 * leaves `in` unchanged.  vals_out (optional): vals[v k + j] = p_v(z_j), the remainder in evaluation form. */
int msm_amd_fr_poly_div_points(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* z /* k HOST records */, size_t k,
                               const void* in, size_t n, size_t n_vec, void* out, void* vals_out /* HOST memory, optional */,
                               float* kernel_ms);
/* The twins: the division is upstream's shape, k chained divisions by X - z_j, and the values come from k evaluations -- a
 * different algorithm from the device's partial fractions.  The bytes do not depend on `threads`. */
int msm_amd_host_fr_poly_eval_points(int scalar_layout, const void* z, size_t k, const void* coeffs, size_t n, size_t n_vec,
                                     int threads, void* y_out);
int msm_amd_host_fr_poly_div_points(int scalar_layout, const void* z, size_t k, const void* in, size_t n, size_t n_vec,
                                    int threads, void* out, void* vals_out);
/* Test aid (no ctx, CPU only): the plan of a call at k points and a tile of 2^tile_log (2 .. 9).  counts: [0] launches (those
 * of one point), [1] waves over all launches, [2] records and [3] bytes of ctx-owned device memory, [4] levels, [5] bytes
 * of the kernel arguments of a level-0 launch (< 4096), [6] waves of the level-0 launches, [7] 0. */
int msm_amd_test_fr_poly_points_plan(size_t n, size_t n_vec, size_t k, uint32_t tile_log, int divide, uint64_t counts[8]);

/* ---- gate polynomials over rotated columns: sums of products, row by row ---------------------------------------
 * The quotient numerator on the extended coset (halo2 evaluate_h; the gate and copy-constraint sums of a PLONK prover):
 * n_vec columns of n records, column v at in + 32 v stride, and for every row 0 <= i < n
 *     v[i]   = sum_k c_k prod_j col_(factors[k][j])[(i + rotations[k][j] rot_step) mod n]
 *     out[i] = v[i]                                  plain
 *     out[i] = k_acc out[i] + v[i]                   MSM_AMD_GATE_ACCUMULATE: halo2's values * y + gate
 *     out[i] = (either of the above) scale[i mod period]      scale given: the periodic 1 / Z_H
 * Up to 256 columns, 16 terms, 8 factors per term; an index may repeat inside a term (powers) and across terms.  The
 * effective offset of a factor is (rot rot_step) mod n with the non-negative remainder, for any int32 rot and any
 * rot_step >= 1 (2^(extended_k - k) on an extended domain); a call may use at most MSM_AMD_GATE_MAX_OFFSETS DISTINCT
 * effective offsets.  The host reduces them once; what travels to the kernel by value is the 8 offsets and, per factor, a
 * column byte and an offset-slot byte: a row costs one addition and one conditional subtraction.  The coefficients are
 * records in HOST memory in the call's layout, any 256-bit word taken mod r; 1 and r - 1 cost no product.
 * Records, layouts, "any word mod r", fully reduced outputs (unique bytes), 16-byte alignment of device pointers, the
 * bounded wait, the busy-ctx error and msm_amd_last_error are those of msm_amd_fr_map*.  Any n >= 1 below 2^32 (not only
 * powers of two), stride >= n, n_vec stride < 2^32.  n == 0 or n_vec == 0: MSM_AMD_OK, nothing is touched, the term list is
 * not looked at.  One launch per call, one lane per row.
 * out: n records, disjoint from the whole input span (an overlap is MSM_AMD_INPUT_ERROR: rotated reads make in-place
 * evaluation meaningless); without ACCUMULATE its old bytes are never read; the input is never written.
 * MSM_AMD_INPUT_ERROR, each with its own text and no byte of out written: n_terms outside 1 .. 16; a term length outside
 * 1 .. 8; a column index not below n_vec; n_vec above 256; more than 8 distinct offsets; rot_step == 0; n >= 2^32; a period
 * that is no power of two in 1 .. 256 or does not divide n; an unknown flag, mem or layout; stride < n; a null pointer the
 * call reads (k_acc32 only with ACCUMULATE); a device pointer that is not 16-byte aligned; an overlap of out and in. */
enum { MSM_AMD_GATE_MAX_COLUMNS = 256, MSM_AMD_GATE_MAX_TERMS = 16, MSM_AMD_GATE_MAX_FACTORS = 8, MSM_AMD_GATE_MAX_OFFSETS = 8,
       MSM_AMD_GATE_MAX_PERIOD = 256 };
enum { MSM_AMD_GATE_ACCUMULATE = 1 };   /* flags */
typedef struct msm_amd_fr_gate_terms {
  uint32_t n_terms;          /* 1 .. 16 */
  const void* coeff;         /* n_terms records, HOST memory, the call's scalar layout, any 256-bit word taken mod r */
  const uint32_t* term_len;  /* n_terms values, each 1 .. 8 */
  const uint32_t* factors;   /* sum(term_len) column indices < n_vec, term after term; an index may repeat (powers) */
  const int32_t* rotations;  /* one per factor, any value */
} msm_amd_fr_gate_terms;
/* The check of a term list every entry point shares (no ctx, CPU only; the coefficients are not read): the longest term in
 * *degree and the number of distinct effective offsets in *n_offsets (both optional).  MSM_AMD_INPUT_ERROR for a list the
 * calls below refuse, n_vec == 0 and n == 0 included; msm_amd_fr_gate_last_error has the text. */
int msm_amd_fr_gate_check(const msm_amd_fr_gate_terms* terms, size_t n_vec, size_t n, uint64_t rot_step, uint32_t* degree,
                          uint32_t* n_offsets);
/* Why the last msm_amd_fr_gate_check, msm_amd_host_fr_gate_eval or msm_amd_test_fr_gate_plan of the calling thread
 * refused its arguments ("" after a call that did not): the calls without a ctx have no msm_amd_last_error. */
const char* msm_amd_fr_gate_last_error(void);
/* mem (MSM_AMD_MEM_HOST / MSM_AMD_MEM_DEVICE, below): where in and out lie -- host memory staged through the ctx like the
 * other host-buffer forms, or device-resident columns.  k_acc32 (one record) and scale (period records; NULL: no
 * scaling, period is ignored) are HOST memory either way, in the call's layout; the scale table goes to ctx-owned device
 * memory (period 32 bytes).  kernel_ms is optional. */
int msm_amd_fr_gate_eval(msm_amd_ctx* ctx, int mem, int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms,
                         const void* in, size_t n, size_t n_vec, size_t stride, uint64_t rot_step,
                         const void* k_acc32 /* HOST memory */, const void* scale /* HOST memory, optional */, size_t period,
                         void* out, float* kernel_ms);
/* The same on the CPU (no ctx, no GPU; the same bodies compiled for the host); threads <= 0: up to 16 host threads. */
int msm_amd_host_fr_gate_eval(int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms, const void* in, size_t n,
                              size_t n_vec, size_t stride, uint64_t rot_step, const void* k_acc32, const void* scale,
                              size_t period, int threads, void* out);
/* Test aid (no ctx, CPU only): the plan of a call; period == 0: no scale.  counts: [0] launches (1), [1] workgroups,
 * [2] records read per row (the factors, the old output of ACCUMULATE, the scale), [3] field products per row: len - 1 per
 * term, one for a coefficient that is neither 1 nor r - 1, one each for ACCUMULATE and the scale, [4] distinct offsets,
 * [5] bytes of ctx-owned device memory (the scale table, else 0), [6] the degree, [7] 0. */
int msm_amd_test_fr_gate_plan(int scalar_layout, uint32_t flags, const msm_amd_fr_gate_terms* terms, size_t n, size_t n_vec,
                              uint64_t rot_step, size_t period, uint64_t counts[8]);

/* ---- sparse matrix times vector over Fr: the R1CS witness map ------------------------------------------------
 * Every R1CS prover starts from A z, B z, C z: three sparse matrices over Fr, fixed per circuit, times the assignment of
 * one proof (arkworks witness_map_from_matrices; the same step in snarkjs and bellman; Marlin and Spartan-style provers
 * multiply sparse matrices over Fr as well).  A matrix is built once per key and lives on the device; a product reads x
 * and writes y where the transforms and the Fr vector calls work.
 *   y[i] = sum_{k in [row_ptr[i], row_ptr[i+1])} values[k] x[col_idx[k]] mod r,   i < n_rows
 * The matrix is CSR in HOST memory: row_ptr of n_rows + 1 offsets, col_idx and values of nnz = row_ptr[n_rows] entries.  A
 * row may be empty (y[i] = 0); a column may repeat within a row (the terms add); an explicit zero value is legal.
 * Records as in the Fr vector calls: MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE (MSM_AMD_SCALAR_CANON_BE32:
 * MSM_AMD_INPUT_ERROR), any 256-bit word is taken mod r, every y[i] is the fully reduced residue -- the bytes of y are
 * unique and depend on no order of summation, plan or thread count.  The layout of `values` is fixed at the build; the
 * layout of x and y is chosen per call; the handle keeps Montgomery residues.
 * msm_amd_fr_matrix_build: MSM_AMD_INPUT_ERROR for a null pointer (col_idx and values may be null only with nnz == 0),
 * n_rows == 0, n_cols == 0, n_rows or n_cols or nnz >= 2^32, row_ptr[0] != 0, a decreasing row_ptr and any col_idx[k] >=
 * n_cols -- every column is checked on the host before anything is uploaded, so a bad matrix never becomes a wild read
 * on the device.  The values are reduced and deduplicated (r + 1 and 1 share an entry; R1CS values are mostly +-1): the
 * device holds 8 bytes per entry -- column and dictionary id -- and 32 per distinct value; n_distinct and the size of the
 * one allocation come back from msm_amd_fr_matrix_info, where any out pointer may be null.  msm_amd_destroy releases the
 * handles the caller did not free.
 * msm_amd_fr_matvec*: MSM_AMD_INPUT_ERROR for a pointer that is not a live matrix handle of this ctx (a transform domain
 * or a table handle is none; a freed handle neither), a null x or y, a device pointer that is not 16-byte aligned, a y
 * that overlaps x in any way (the product is out of place only: a row gathers from all of x), and d_x or d_y overlapping
 * the matrix.  The calls serialise on the ctx and wait -- bounded -- for its earlier work (a busy ctx:
 * MSM_AMD_PIPELINE_ERROR, msm_amd_last_error names the call); the host-buffer form uploads x through the page-locked
 * staging ring and copies y back; kernel_ms (optional) is the device time of the kernels.
 * On the device short rows take one lane each, longer rows one wave per segment, and a row of several segments leaves
 * partial sums in ctx-owned memory that a last launch folds: one to three launches in stream order, nothing waits on
 * another workgroup.  (Development knobs at msm_amd_init: MSM_AMD_FR_MAT_LONG = 1 .. 4096, rows above this many entries
 * leave the lane path, default 32; MSM_AMD_FR_MAT_SEG_LOG = 6 .. 20, entries per wave of the other path as a power of
 * two, default 8 (measured: profiles/fr_mat_ab.txt); MSM_AMD_FR_MAT_SIGNS = 0 / 1, the kernels that add and subtract
 * entries of value 1 and r - 1 without a product, default 0.  A matrix is planned at its build.  No byte of a result
 * depends on any of them.) */
typedef struct msm_amd_fr_matrix msm_amd_fr_matrix;
int msm_amd_fr_matrix_build(msm_amd_ctx* ctx, int scalar_layout, size_t n_rows, size_t n_cols,
                            const uint64_t* row_ptr /* n_rows + 1 */, const uint32_t* col_idx /* nnz */,
                            const void* values /* nnz x 32 B */, msm_amd_fr_matrix** out); /* all HOST memory */
int msm_amd_fr_matrix_info(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, size_t* n_rows, size_t* n_cols, size_t* nnz,
                           size_t* n_distinct, size_t* device_bytes);
int msm_amd_fr_matrix_free(msm_amd_ctx* ctx, msm_amd_fr_matrix* matrix);
int msm_amd_fr_matvec(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, int scalar_layout, const void* x, void* y);
int msm_amd_fr_matvec_device(msm_amd_ctx* ctx, const msm_amd_fr_matrix* matrix, int scalar_layout, const void* d_x, void* d_y,
                             float* kernel_ms);
/* The same on the CPU (no ctx, no GPU): scalar_layout is that of values, x and y; the same argument checks; rows go to
 * the threads in ranges of equal entry count; threads <= 0: up to 16 host threads. */
int msm_amd_host_fr_matvec(int scalar_layout, size_t n_rows, size_t n_cols, const uint64_t* row_ptr, const uint32_t* col_idx,
                           const void* values, const void* x, int threads, void* y);
/* Test aid (no ctx, CPU only): the plan of a matrix with these row offsets at long_rows (1 .. 4096) and seg_log (6 .. 20).
 * counts: [0] lane rows, [1] wave rows, [2] segments, [3] split rows, [4] partial records, [5] launches (1, 2 or 3), [6]
 * dispatched waves (one per 64 consecutive rows, one per segment, one per split row), [7] 0.  segs (may be null with
 * segs_cap == 0) receives the first segs_cap segment records of four words: row, first entry, entry count, partial slot
 * (0xFFFFFFFF: the segment is its whole row and stores to y).  The other test aid of these calls is
 * msm_amd_test_fill_workspaces: it poisons the partial records too. */
int msm_amd_test_fr_matrix_plan(size_t n_rows, const uint64_t* row_ptr, uint32_t long_rows, uint32_t seg_log,
                                uint64_t counts[8], uint32_t* segs, size_t segs_cap);

/* ---- multilinear tables over Fr and the rounds of a sumcheck ---------------------------------------------------
 * Spartan, HyperPlonk, Nova / HyperNova and GKR-style provers spend their time between the MSMs in the sumcheck protocol
 * over multilinear tables: each round sums a low-degree combination of a few tables, takes a challenge and halves every
 * table.  These calls do that on the device, where msm_amd_fr_matvec_device leaves A z, B z, C z.
 * A table is n = 2^m records f[i], the value at x = (x_0 .. x_(m-1)) with x_j = bit j of i.  Records, layouts
 * (MSM_AMD_SCALAR_MONT_LE, _CANON_LE; _CANON_BE32: MSM_AMD_INPUT_ERROR), "any 256-bit word is taken mod r", fully reduced
 * outputs (unique bytes), 16-byte alignment of device pointers, the bounded waits and msm_amd_last_error are those of
 * msm_amd_fr_prefix_product*.  n_vec tables lie `stride` records apart (stride >= n, n_vec stride < 2^32).  Challenges and
 * points are records in HOST memory in the call's layout, for every form of every call; y_out and g_out are HOST memory too
 * and come back through ctx-owned page-locked memory in the call's one bounded wait.
 * Two orders, because both are in use:
 *   MSM_AMD_MLE_LOW   step s binds x_s:        f'[i] = f[2i] + r (f[2i+1] - f[2i]), i < n/2  (arkworks
 *                     DenseMultilinearExtension::fix_variables)
 *   MSM_AMD_MLE_HIGH  step s binds x_(m-1-s):  f'[i] = f[i] + r (f[i + n/2] - f[i])           (Spartan / Nova
 *                     bound_poly_var_top)
 * Sizes and errors: n a power of two, 2 <= n < 2^32.  n_vec == 0: MSM_AMD_OK, nothing is touched.  MSM_AMD_INPUT_ERROR: n
 * not a power of two or < 2; n_bind == 0 or > m; stride < n; n_vec stride >= 2^32; an unknown order, form or layout; n_vec
 * outside a form's range; a null pointer the call reads or writes; misaligned device pointers; the overlap rules of
 * msm_amd_fr_mle_bind*.  The host twins msm_amd_host_fr_* (no ctx, no GPU; the same bodies compiled for the host) make
 * the same checks; threads <= 0: up to 16 host threads; no byte depends on the thread count.
 * (Development knob at msm_amd_init: MSM_AMD_FR_MLE_CHUNK_LOG = 6 .. 20, the pairs per wave of a round as a power of two,
 * default 8 (measured: profiles/mle_ab.txt); the evaluation runs on the tiles of MSM_AMD_FR_TILE_LOG.  No byte of a result
 * depends on either.) */
enum { MSM_AMD_MLE_LOW = 0, MSM_AMD_MLE_HIGH = 1 };
enum { MSM_AMD_SUMCHECK_PRODUCT = 0,   /* F = prod_j f_j, n_vec 1 .. 4, d = n_vec */
       MSM_AMD_SUMCHECK_EQ_AB_C = 1    /* n_vec = 4, tables eq, a, b, c: F = eq (a b - c), d = 3 */ };
/* n_bind steps (1 <= n_bind <= m) with r[0], r[1], .. on each table.  The first n >> n_bind records of output table v (at
 * out + 32 v stride) are the result; the call may also write the rest of that table's first n/2 records (unspecified
 * content) and writes no other byte of out.  out == in is allowed with MSM_AMD_MLE_HIGH; otherwise out must be disjoint
 * from the whole input span of (n_vec - 1) stride + n records: MSM_AMD_MLE_LOW is out of place only, a partial overlap is
 * MSM_AMD_INPUT_ERROR.  An out-of-place call leaves `in` unchanged.  One launch folds up to three variables; LOW with more
 * than one launch uses ctx-owned memory of n_vec n / 8 records. */
int msm_amd_fr_mle_bind(msm_amd_ctx* ctx, int scalar_layout, int order, const void* r /* n_bind records */, size_t n_bind,
                        const void* in, size_t n, size_t n_vec, size_t stride, void* out);
int msm_amd_fr_mle_bind_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* r /* HOST memory */, size_t n_bind,
                               const void* d_in, size_t n, size_t n_vec, size_t stride, void* d_out, float* kernel_ms);
int msm_amd_host_fr_mle_bind(int scalar_layout, int order, const void* r, size_t n_bind, const void* in, size_t n, size_t n_vec,
                             size_t stride, int threads, void* out);
/* y[v] = the one record left of table v after m steps at point[0 .. m-1]; `in` is never written.  HIGH at a point equals
 * LOW at the reversed point. */
int msm_amd_fr_mle_eval(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point /* m records */, const void* in,
                        size_t n, size_t n_vec, size_t stride, void* y_out /* n_vec records */);
int msm_amd_fr_mle_eval_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point /* HOST memory */,
                               const void* d_in, size_t n, size_t n_vec, size_t stride, void* y_out /* HOST memory */,
                               float* kernel_ms);
int msm_amd_host_fr_mle_eval(int scalar_layout, int order, const void* point, const void* in, size_t n, size_t n_vec,
                             size_t stride, int threads, void* y_out);
/* out[i] = prod_s (bit v(s) of i ? point[s] : 1 - point[s]), i < 2^m, with v(s) = s for LOW and m - 1 - s for HIGH;
 * 1 <= m <= 31.  eval(f, order, point) = sum_i out[i] f[i]. */
int msm_amd_fr_eq_table(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point /* m records */, size_t m, void* out);
int msm_amd_fr_eq_table_device(msm_amd_ctx* ctx, int scalar_layout, int order, const void* point /* HOST memory */, size_t m,
                               void* d_out /* 2^m records */, float* kernel_ms);
int msm_amd_host_fr_eq_table(int scalar_layout, int order, const void* point, size_t m, int threads, void* out);
/* One round's polynomial.  With h = n/2 and (lo_j(x), hi_j(x)) the two records of table j that the next step of `order`
 * would combine at output index x (LOW: 2x, 2x + 1; HIGH: x, x + h), f_j(t, x) = lo_j + t (hi_j - lo_j) and
 *   g_out[t] = sum_(x < h) F(f_0(t, x), ..),  t = 0 .. d, t an integer mod r.
 * All d + 1 values come back, g(1) included, so that a caller can check g(0) + g(1) against its claim.  `in` is never
 * written.  PRODUCT with one table is the sum of a table, with two an inner product (Spartan's second sumcheck); EQ_AB_C
 * is Spartan's first sumcheck, the R1CS zero check. */
int msm_amd_fr_sumcheck_round(msm_amd_ctx* ctx, int scalar_layout, int order, int form, const void* in, size_t n, size_t n_vec,
                              size_t stride, void* g_out /* d + 1 records */);
int msm_amd_fr_sumcheck_round_device(msm_amd_ctx* ctx, int scalar_layout, int order, int form, const void* d_in, size_t n,
                                     size_t n_vec, size_t stride, void* g_out /* HOST memory */, float* kernel_ms);
int msm_amd_host_fr_sumcheck_round(int scalar_layout, int order, int form, const void* in, size_t n, size_t n_vec, size_t stride,
                                   int threads, void* g_out);
/* Test aid (no ctx, CPU only): the plan of one of these calls at chunk_log (6 .. 20) and tile_log (2 .. 9).  For the eq
 * table n is m; the plan of a bind or an eval takes the tables at stride n.  counts: [0] launches, [1] dispatched waves,
 * [2] records of ctx-owned device memory, [3] the same in bytes, [4] levels (round: 1 + fold launches; eval: launches),
 * [5] waves of the first launch of a round or an eval, [6] records the call defines (round: d + 1), [7] 0.
 * msm_amd_test_fill_workspaces poisons the partial records and the levels of these calls too. */
enum { MSM_AMD_MLE_CALL_BIND = 0, MSM_AMD_MLE_CALL_EVAL = 1, MSM_AMD_MLE_CALL_EQ_TABLE = 2, MSM_AMD_MLE_CALL_ROUND = 3 };
int msm_amd_test_fr_mle_plan(int call, int order, int form, size_t n, size_t n_vec, uint32_t n_bind, uint32_t chunk_log,
                             uint32_t tile_log, uint64_t counts[8]);

/* ---- sumcheck rounds over a caller-described sum of products, and the step that binds first ----------------------
 * arkworks' ListOfProductsOfPolynomials, HyperPlonk's gate zero checks and GKR layers are sums of products of tables
 * under an optional common factor:
 *   F = [f_outer] sum_k c_k prod_j f_(factors[k][j]),   d = max_k term_len[k] + (outer given ? 1 : 0),   1 <= d <= 7.
 * Up to 16 tables, 16 terms, 6 factors per term; an index may repeat inside a term (powers) and across terms, and the
 * outer table may also be a factor.  The coefficients are records in HOST memory in the call's layout, any 256-bit
 * word taken mod r; 1 and r - 1 cost no product.  Tables, stride, orders, layouts, "any word mod r", fully reduced
 * outputs, alignment, the bounded wait and msm_amd_last_error are those of msm_amd_fr_sumcheck_round*; g_out is HOST
 * memory, d + 1 records g(0) .. g(d).  n_vec == 0: MSM_AMD_OK, nothing is touched, the term list is not looked at.
 * MSM_AMD_INPUT_ERROR, each with its own text: n_terms outside 1 .. 16; a term length outside 1 .. 6; a table index
 * (outer included) not below n_vec; n_vec above 16; a null pointer in the list or a null list. */
enum { MSM_AMD_SUMCHECK_MAX_TABLES = 16, MSM_AMD_SUMCHECK_MAX_TERMS = 16, MSM_AMD_SUMCHECK_MAX_FACTORS = 6 };
#define MSM_AMD_SUMCHECK_NO_OUTER 0xFFFFFFFFu
typedef struct msm_amd_fr_sumcheck_terms {
  uint32_t n_terms;          /* 1 .. 16 */
  uint32_t outer;            /* a table index < n_vec, or MSM_AMD_SUMCHECK_NO_OUTER */
  const void* coeff;         /* n_terms records, HOST memory, the call's scalar layout, any 256-bit word taken mod r */
  const uint32_t* term_len;  /* n_terms values, each 1 .. 6 */
  const uint32_t* factors;   /* sum(term_len) table indices < n_vec, term after term; an index may repeat (powers) */
} msm_amd_fr_sumcheck_terms;
/* The shared check of a term list against n_vec tables (no ctx, CPU only; the coefficients are not read) and its
 * degree in *d.  MSM_AMD_INPUT_ERROR for a list the calls below refuse, n_vec == 0 and a null d included. */
int msm_amd_fr_sumcheck_terms_degree(const msm_amd_fr_sumcheck_terms* terms, size_t n_vec, uint32_t* d);
/* One round's polynomial of F, as msm_amd_fr_sumcheck_round*: `in` is never written.  mem (MSM_AMD_MEM_HOST /
 * MSM_AMD_MEM_DEVICE, below): where `in` lies -- host memory staged through the ctx like the other host-buffer forms, or
 * device-resident tables, 16-byte aligned; an unknown mem is MSM_AMD_INPUT_ERROR.  (One entry point with a `mem` argument
 * rather than a _device twin, as msm_amd_fr_sort: DESIGN.md section 8.16.)  g_out is HOST memory either way; kernel_ms is
 * optional. */
int msm_amd_fr_sumcheck_round_terms(msm_amd_ctx* ctx, int mem, int scalar_layout, int order,
                                    const msm_amd_fr_sumcheck_terms* terms, const void* in, size_t n, size_t n_vec,
                                    size_t stride, void* g_out /* d + 1 HOST records */, float* kernel_ms);
int msm_amd_host_fr_sumcheck_round_terms(int scalar_layout, int order, const msm_amd_fr_sumcheck_terms* terms, const void* in,
                                         size_t n, size_t n_vec, size_t stride, int threads, void* g_out);
/* One step of a sumcheck in one call and one bounded wait: bind the previous round's challenge r (one HOST record),
 * then the next round's values (a bind launch and the round's launches on the ctx's stream).  By definition the result is that of
 * msm_amd_fr_mle_bind*(n_bind = 1, r) followed by msm_amd_fr_sumcheck_round_terms* at n / 2 on the bound tables: the
 * first n / 2 records of every output table (at out + 32 v stride) are the bound table, fully reduced, in the call's
 * layout, and g_out is that table set's round polynomial.  The call writes NO OTHER BYTE of out (stricter than bind).
 * n a power of two, n >= 4: the last variable is msm_amd_fr_mle_bind / msm_amd_fr_mle_eval.  MSM_AMD_MLE_HIGH: out ==
 * in is allowed; otherwise out must be disjoint from the whole input span.  MSM_AMD_MLE_LOW is out of place only; a
 * partial overlap is MSM_AMD_INPUT_ERROR.  An out-of-place call leaves `in` unchanged.  A whole sumcheck of m
 * variables: round_terms once, step_terms per challenge but the last, mle_eval or mle_bind for the last variable. */
int msm_amd_fr_sumcheck_step_terms(msm_amd_ctx* ctx, int mem /* of in and out */, int scalar_layout, int order,
                                   const msm_amd_fr_sumcheck_terms* terms, const void* r /* HOST memory */, const void* in,
                                   size_t n, size_t n_vec, size_t stride, void* out, void* g_out /* d + 1 HOST records */,
                                   float* kernel_ms);
int msm_amd_host_fr_sumcheck_step_terms(int scalar_layout, int order, const msm_amd_fr_sumcheck_terms* terms, const void* r,
                                        const void* in, size_t n, size_t n_vec, size_t stride, int threads, void* out,
                                        void* g_out);
/* Test aid (no ctx, CPU only): the plan of one of these calls at chunk_log (6 .. 20); step != 0: the step call at n.
 * counts as the round row of msm_amd_test_fr_mle_plan: [0] launches, [1] dispatched waves, [2] records of ctx-owned
 * device memory, [3] the same in bytes, [4] levels, [5] waves of the first launch, [6] d + 1, [7] 0. */
int msm_amd_test_fr_sumcheck_terms_plan(const msm_amd_fr_sumcheck_terms* terms, size_t n, size_t n_vec, uint32_t chunk_log,
                                        int step, uint64_t counts[8]);

/* ---- Poseidon over Fr: permutations, hashes and Merkle trees ------------------------------------------------------------
 * The algebraic hash of the circomlib / circomlibjs / iden3 family (Grassi et al., S-box x^5) over BN254 Fr for a state of
 * t = 2 .. 5 records: Semaphore / Tornado style membership trees, Poseidon-Merkle commitments to columns that
 * msm_amd_ntt_device or msm_amd_fr_matvec_device leave on the device, the commitment hashes of Nova / Spartan style provers.
 * The textbook schedule, rounds 0-based, for rho < r_f + r_p:
 *   s[i] += ark[rho t + i];  s[i] = s[i]^5 for every i when rho < r_f/2 or rho >= r_f/2 + r_p, else for i = 0 only;
 *   s'[i] = sum_j mds[i t + j] s[j].
 * Records, layouts (MSM_AMD_SCALAR_MONT_LE, _CANON_LE; anything else: MSM_AMD_INPUT_ERROR), "any 256-bit word is taken mod
 * r", fully reduced outputs (unique bytes), 16-byte alignment of device pointers, the bounded waits and msm_amd_last_error
 * are those of msm_amd_fr_map*.  Every call serialises on the ctx.  A count of 2^32 or more is MSM_AMD_INPUT_ERROR; n == 0
 * (n_idx == 0) is MSM_AMD_OK and touches nothing.  The host twins msm_amd_host_poseidon_* (no ctx, no GPU; the same bodies
 * compiled for the host) take the constants directly and make the same checks; threads <= 0: up to 16 host threads; no
 * byte depends on the thread count.
 * (Development knob at msm_amd_init: MSM_AMD_POSEIDON_TOP_LOG = 0 .. 10, default 8 (profiles/poseidon_ab.txt): the levels
 * of a tree of at most 2^TOP nodes run in one workgroup.  No byte of a result depends on it.) */
typedef struct msm_amd_poseidon_params msm_amd_poseidon_params;
/* The constants of the Poseidon paper's reference generator (generate_parameters_grain: field 1, S-box 0, 254 bits) for
 * (t, r_f, r_p): (r_f + r_p) t round constants into ark_out and the t x t matrix, row-major, into mds_out, as records of
 * scalar_layout.  With r_f = 8 and r_p = 56, 57, 56, 60 for t = 2, 3, 4, 5 these are circomlib's.  Pure host call.
 * MSM_AMD_INPUT_ERROR: t outside 2 .. 5, r_f odd or zero, r_f + r_p > 128, a null output, an unknown layout. */
int msm_amd_poseidon_constants(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, void* ark_out, void* mds_out);
/* Constants of the caller (or of msm_amd_poseidon_constants) in host memory -> a handle that keeps their Montgomery residues
 * in one device allocation.  msm_amd_destroy frees the handles the caller left.  In every call below a handle of another
 * kind or of another ctx, or a freed one, is MSM_AMD_INPUT_ERROR. */
int msm_amd_poseidon_params_build(msm_amd_ctx* ctx, uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark,
                                  const void* mds, msm_amd_poseidon_params** out);
int msm_amd_poseidon_params_info(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, uint32_t* t, uint32_t* r_f,
                                 uint32_t* r_p, size_t* device_bytes);   /* any output pointer may be null */
int msm_amd_poseidon_params_free(msm_amd_ctx* ctx, msm_amd_poseidon_params* params);
/* n states of t records, back to back -> n states.  out == in is allowed, a partial overlap is MSM_AMD_INPUT_ERROR. */
int msm_amd_poseidon_permute(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* in, size_t n,
                             void* out);
int msm_amd_poseidon_permute_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* d_in,
                                    size_t n, void* d_out, float* kernel_ms);
int msm_amd_host_poseidon_permute(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                                  const void* in, size_t n, int threads, void* out);
/* n groups of t - 1 records -> n digests: state = [tag, in_0 .. in_(t-2)], digest = word 0 of the permuted state.  tag32 is
 * one record in HOST memory; null is 0, which gives circomlib's poseidon([...]).  out == in is allowed for t = 2 only, where
 * digest i replaces the one record it was computed from.  For t >= 3 digest i would land on a record of group i / (t - 1),
 * which another lane reads, and nothing orders the lanes of two workgroups: there `out` must be disjoint from all of `in`,
 * any overlap is MSM_AMD_INPUT_ERROR. */
int msm_amd_poseidon_hash(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* tag32,
                          const void* in, size_t n, void* out);
int msm_amd_poseidon_hash_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout,
                                 const void* tag32 /* HOST memory */, const void* d_in, size_t n, void* d_out, float* kernel_ms);
int msm_amd_host_poseidon_hash(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                               const void* tag32, const void* in, size_t n, int threads, void* out);
/* The tree of arity a = t - 1 (t >= 3) over n_leaves = a^d leaves, d >= 1; any other count is MSM_AMD_INPUT_ERROR: padding is
 * the caller's policy.  Leaves are field elements and are not written.  `tree` receives the (a^d - 1) / (a - 1) inner nodes
 * level by level, the parents of the leaves first, the root last; a node is the hash of its a children under tag32.  A
 * tree that overlaps the leaves is MSM_AMD_INPUT_ERROR.  root32: optional, 32 bytes of HOST memory for the root. */
int msm_amd_poseidon_merkle_build(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* tag32,
                                  const void* leaves, size_t n_leaves, void* tree, void* root32);
int msm_amd_poseidon_merkle_build_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout,
                                         const void* tag32 /* HOST memory */, const void* d_leaves, size_t n_leaves,
                                         void* d_tree, void* root32 /* HOST memory */, float* kernel_ms);
int msm_amd_host_poseidon_merkle_build(uint32_t t, uint32_t r_f, uint32_t r_p, int scalar_layout, const void* ark, const void* mds,
                                       const void* tag32, const void* leaves, size_t n_leaves, int threads, void* tree,
                                       void* root32);
/* The authentication paths of n_idx leaves of such a tree.  idx: leaf indices in HOST memory for every form; an index >=
 * n_leaves is MSM_AMD_INPUT_ERROR, found before anything is launched.  out: d (a - 1) sibling records per index, the level
 * of the leaves first, the siblings of a level in child order with the node's own place left out; n_idx d (a - 1) < 2^32.
 * out must not overlap leaves or tree. */
int msm_amd_poseidon_merkle_paths(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout, const void* leaves,
                                  size_t n_leaves, const void* tree, const uint64_t* idx, size_t n_idx, void* out);
int msm_amd_poseidon_merkle_paths_device(msm_amd_ctx* ctx, const msm_amd_poseidon_params* params, int scalar_layout,
                                         const void* d_leaves, size_t n_leaves, const void* d_tree,
                                         const uint64_t* idx /* HOST memory */, size_t n_idx, void* d_out, float* kernel_ms);
int msm_amd_host_poseidon_merkle_paths(uint32_t t, int scalar_layout, const void* leaves, size_t n_leaves, const void* tree,
                                       const uint64_t* idx, size_t n_idx, int threads, void* out);
/* Test aid (no ctx, CPU only): the launches of a tree build at top_log (0 .. 10).  counts: [0] launches, [1] d, [2] inner
 * nodes, [3] levels of the last workgroup, [4] its nodes, [5 .. 7] 0, [8 + k] nodes of launch k (the last: counts[4]). */
int msm_amd_test_poseidon_plan(uint32_t t, size_t n_leaves, uint32_t top_log, uint64_t counts[40]);

/* Test aid (no ctx): the plan of a scan over n_vec vectors of n at a tile of 2^tile_log (2 .. 9): out[0] levels, out[1]
 * launches (2 levels - 1), out[2] tiles of the first level over all vectors, out[3] records of ctx-owned device memory */
int msm_amd_test_fr_plan(size_t n, size_t n_vec, uint32_t tile_log, uint64_t out[4]);

/* ---- lookup arguments over Fr: multiplicities and row indices ------------------------------------------------------------
 * A log-derivative lookup (logUp) needs m[j] = #{ i : f[i] = t[j] }: Fr values matched against Fr values.  A table is one
 * column of n_rows 32-byte records, 1 <= n_rows < 2^31 (n_rows == 0: MSM_AMD_INPUT_ERROR), MSM_AMD_SCALAR_MONT_LE or
 * MSM_AMD_SCALAR_CANON_LE, any 256-bit word taken mod r; a table of tuples is the caller's theta-compression
 * (msm_amd_fr_lincomb_device).  The handle keeps its own reduced copy of the rows -- the caller's buffer is not referenced
 * after the build returns -- and an open-addressing index with linear probing over them: a power of two of 32-bit slots, at
 * least 2 n_rows, hashed over all eight words of the residue.  Rows that are equal mod r share one slot, and their
 * representative is the SMALLEST row index, whatever the order the rows arrive in.  Every probe loop is bounded by the
 * capacity; one that runs out (it cannot at this load) is MSM_AMD_PIPELINE_ERROR with a message, not a hang.
 * msm_amd_fr_lookup_build_device is cheap enough for a table that depends on a per-proof challenge: one reduce-and-copy
 * pass, one insert pass, one bounded wait that also brings the numbers of msm_amd_fr_lookup_info (longest_probe: the most
 * slots one insert looked at).  Lifetime and misuse as for msm_amd_fr_matrix_*: bound to its ctx, a freed or foreign handle
 * is MSM_AMD_INPUT_ERROR, msm_amd_destroy frees what is left.
 * (Development knobs, read at every call: MSM_AMD_LOOKUP_HASH_BITS = 0 .. 32, default all: only that many bits of the hash
 * choose the home slot, homes are taken from the top of the slot array so that chains wrap, 0 is one chain from the last
 * slot; MSM_AMD_LOOKUP_COUNT = block (default: one atomic per distinct row per wave, the largest group of each of a
 * workgroup's 16 waves folded through LDS first), wave (without the fold) or lane (one atomic per input).  No byte of any
 * output depends on either.) */
typedef struct msm_amd_fr_lookup msm_amd_fr_lookup;
int msm_amd_fr_lookup_build(msm_amd_ctx* ctx, int scalar_layout, const void* table, size_t n_rows, msm_amd_fr_lookup** out);
int msm_amd_fr_lookup_build_device(msm_amd_ctx* ctx, int scalar_layout, const void* d_table, size_t n_rows,
                                   msm_amd_fr_lookup** out, float* kernel_ms);
/* every out pointer is optional */
int msm_amd_fr_lookup_info(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, size_t* n_rows, size_t* n_distinct,
                           size_t* capacity, size_t* device_bytes, size_t* longest_probe);
int msm_amd_fr_lookup_free(msm_amd_ctx* ctx, msm_amd_fr_lookup* lookup);
/* n_vec columns of n records back to back, all looked up in the one table; n n_vec < 2^32.
 * m_out[j] (n_rows records): the number of inputs equal to row j mod r as a fully reduced record in scalar_layout, credited
 * to the representative only -- duplicate rows further down get 0 (any split satisfies logUp's identity; this one is
 * deterministic).  idx_out (optional, n n_vec words): the representative's row index of every input, 0xFFFFFFFF for a value
 * that is not in the table; written in either mode.  report (HOST memory): { n_missing, first_missing (the smallest flat
 * index, 2^64 - 1 for none), rows_hit, max_multiplicity } -- msm_amd_msm_bounded_device can commit to m at the bit length
 * of report[3] without a width scan.  It comes back in the call's one bounded wait.
 * MSM_AMD_LOOKUP_STRICT: any miss is MSM_AMD_INPUT_ERROR with count and index in msm_amd_last_error (the report is filled
 * in), and m_out is UNTOUCHED: the pass that writes it reads the miss counter on the device.  MSM_AMD_LOOKUP_COUNT_MISSING:
 * MSM_AMD_OK, m counts the hits.  n == 0 or n_vec == 0: MSM_AMD_OK, m all zero, the report zero.
 * MSM_AMD_INPUT_ERROR: an unknown layout or mode; a null in (with inputs), m_out or report; device pointers that are not
 * 16-byte aligned (d_idx_out: 4); m_out or idx_out overlapping in, each other or (device) the table.  The counters live in
 * ctx-owned memory (4 n_rows bytes). */
enum { MSM_AMD_LOOKUP_STRICT = 0, MSM_AMD_LOOKUP_COUNT_MISSING = 1 };
int msm_amd_fr_lookup_multiplicities(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout, int on_missing,
                                     const void* in, size_t n, size_t n_vec, void* m_out, uint32_t* idx_out,
                                     uint64_t report[4]);
int msm_amd_fr_lookup_multiplicities_device(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout,
                                            int on_missing, const void* d_in, size_t n, size_t n_vec, void* d_m_out,
                                            uint32_t* d_idx_out, uint64_t report[4] /* HOST memory */, float* kernel_ms);
/* The same on the CPU, from the table itself (no ctx, no GPU); a miss under STRICT returns MSM_AMD_INPUT_ERROR with the
 * report filled in and m_out untouched */
int msm_amd_host_fr_lookup_multiplicities(int scalar_layout, int on_missing, const void* table, size_t n_rows, const void* in,
                                          size_t n, size_t n_vec, int threads, void* m_out, uint32_t* idx_out,
                                          uint64_t report[4]);
/* Test aid (no ctx): the index of a table of n_rows at hash_bits (0 .. 32): out[0] capacity, out[1] bytes of the device
 * image, out[2] hash bits that choose a home, out[3] byte offset of the slots in the image */
int msm_amd_test_fr_lookup_plan(size_t n_rows, uint32_t hash_bits, uint64_t out[4]);

/* halo2's lookup argument: the permuted columns A', S'.  From an input column A and a table column S of n usable rows the
 * prover of upstream halo2 (zcash, PSE) builds A', a permutation of A, and S', a permutation of S, with A'[0] = S'[0] and
 * A'[i] = S'[i] or A'[i] = A'[i-1] for 0 < i < n, then the product column z[i+1] = z[i] (A[i] + beta)(S[i] + gamma) /
 * ((A'[i] + beta)(S'[i] + gamma)) ("halo2's lookup argument": the calls above this one do the rest).
 * ROW ORDER, NOT VALUE ORDER.  With c[j] the number of inputs of a column whose representative is row j (as for m_out
 * above), off[j] = sum of c[j'] over j' < j, and U the ascending list of the rows with c = 0 (duplicate rows included):
 *   A'  positions off[j] .. off[j] + c[j] - 1 hold row j, for every j with c[j] > 0;
 *   S'  position off[j] holds row j for every j with c[j] > 0; the other positions, ascending, hold rows U[0], U[1], ...
 * halo2's own permute_expression_pair orders A' by ascending field value.  That is another arrangement of the same two
 * multisets, equally valid, and the verifier cannot tell the two apart; halo2's own arrangement is
 * MSM_AMD_PERMUTE_HALO2 of msm_amd_fr_lookup_permute_as below.  Every byte here is determined by the table and the inputs, not by the order in which atomics land.
 * n_vec columns of n records lie back to back; each is permuted on its own against the one table; a_out and s_out are n_vec n
 * records, column by column, fully reduced in scalar_layout.  n n_vec < 2^32 and n_rows n_vec < 2^32.  a_out and s_out are
 * each optional, one must be given; s_out needs n == n_rows (the caller writes the blinding rows behind the n usable
 * ones), without it any n >= 1 goes.  a_out may be `in` itself: the inputs are consumed by the probe launch before
 * anything is written.
 * report: as for msm_amd_fr_lookup_multiplicities*, rows_hit summed over the columns, max_multiplicity the
 * largest counter of any column; it comes back in the call's one bounded wait.  A value that is in no row ALWAYS fails with
 * MSM_AMD_INPUT_ERROR, as halo2 fails the proof: count and index in msm_amd_last_error, the report filled in, BOTH OUTPUTS
 * UNTOUCHED (the kernel that writes them reads the miss counter on the device).  n == 0 or n_vec == 0: MSM_AMD_OK, nothing
 * written, a zero report.
 * MSM_AMD_INPUT_ERROR, before any launch: an unknown layout; a null in (with inputs) or report; neither output; s_out with
 * n != n_rows; a freed or foreign handle; any overlap between in, a_out and s_out other than a_out == in.  After such an
 * argument error the contents of report are undefined (it is filled in for a miss and for MSM_AMD_OK only).  n_rows < 2^31,
 * the limit of the lookup handle; the twin and msm_amd_test_fr_permute_plan refuse more.
 * The buffers are HOST memory and are staged through the ctx like those of the other host-buffer forms; the form on
 * device-resident buffers is msm_amd_fr_lookup_permute_as(.., MSM_AMD_MEM_DEVICE, .., MSM_AMD_PERMUTE_ROWS, ..) below.
 * Ctx-owned memory: 16 bytes per row and column and the tile totals (msm_amd_test_fr_permute_plan).  The scan's tiles are
 * 2^MSM_AMD_PERMUTE_TILE_LOG words (2 .. 11, default 11; read at every call).  MSM_AMD_PERMUTE_FILL=scan finds the row of
 * an output position by a maximum scan instead of the default binary search (4 more bytes per position; the same bytes
 * out). */
int msm_amd_fr_lookup_permute(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int scalar_layout, const void* in, size_t n,
                              size_t n_vec, void* a_out, void* s_out, uint64_t report[4]);
/* The same on the CPU, from the table itself (no ctx, no GPU) */
int msm_amd_host_fr_lookup_permute(int scalar_layout, const void* table, size_t n_rows, const void* in, size_t n, size_t n_vec,
                                   int threads, void* a_out, void* s_out, uint64_t report[4]);
/* Test aid (no ctx): the plan of a call over n_rows rows and n_vec columns at tile_log (2 .. 11): out[0] levels of the scan,
 * out[1] kernels of a call (the probe, 2 levels - 1 of the scan, the fill), out[2] tiles of the first level over all
 * columns, out[3] bytes of ctx-owned memory */
int msm_amd_test_fr_permute_plan(size_t n_rows, size_t n_vec, uint32_t tile_log, uint64_t out[4]);

/* ---- sorting Fr records by canonical value ------------------------------------------------------------------------------------
 * n_vec columns of n records lie back to back; each column is sorted on its own, ascending by the canonical value in [0, r):
 * halo2curves' Ord for Fr, which compares to_repr() from the top byte down.  The key is the residue -- NOT the Montgomery
 * words and NOT the caller's unreduced word: in MSM_AMD_SCALAR_MONT_LE or MSM_AMD_SCALAR_CANON_LE any 256-bit word is taken
 * mod r, and `out` holds fully reduced records of scalar_layout.  The sort is STABLE: records equal mod r keep their input
 * order.  perm_out[v n + k] is the column-relative input index of the record at sorted position k of column v; it ascends
 * within a run of equal values.  out and perm_out are each optional, one must be given; out may be `in` itself.
 * n n_vec < 2^32; n == 0 or n_vec == 0: MSM_AMD_OK, nothing written.  This is the sorted concatenation of plookup, a
 * deduplication or range-table preparation, and the order halo2's permute_expression_pair gives the input column A'.
 * mem.  MSM_AMD_MEM_DEVICE: in, out and perm_out are device pointers, records 16-byte aligned, perm_out 4-byte aligned.
 * MSM_AMD_MEM_HOST: host memory, staged through the ctx like the other host-buffer forms.  (One entry point with a `mem`
 * argument rather than a _device twin: DESIGN.md section 8.16.)  kernel_ms is optional.
 * MSM_AMD_INPUT_ERROR, before any launch: an unknown mem or layout; neither output; n n_vec >= 2^32; a null in with inputs
 * present; a misaligned device pointer; any overlap between in, out and perm_out other than out == in.
 * How it runs.  One pass forms the 32-byte keys in ctx-owned memory and a mask of the key bytes that differ anywhere in the call;
 * the mask comes back in the call's one bounded wait (the call is blocking, as msm_amd_scalar_width*), and a stable 8-bit
 * radix pass then runs only for a byte that differs: columns of small values take 2 to 3 passes, not 32.  No output byte
 * depends on the mask.  Ctx-owned memory: 32 bytes per record, 16 per record of one column, the tile histograms
 * (msm_amd_test_fr_sort_plan); the host form stages 4 more per record when perm_out is asked for. */
enum { MSM_AMD_MEM_HOST = 0, MSM_AMD_MEM_DEVICE = 1 };
int msm_amd_fr_sort(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* in, size_t n, size_t n_vec, void* out,
                    uint32_t* perm_out, float* kernel_ms);
/* The same on the CPU (no ctx, no GPU): a stable merge sort of the indices by the canonical value, on up to `threads` threads */
int msm_amd_host_fr_sort(int scalar_layout, const void* in, size_t n, size_t n_vec, int threads, void* out, uint32_t* perm_out);
/* Test aid (no ctx): the plan of a sort of n_vec columns of n (n, n_vec >= 1, n n_vec < 2^32) whose keys differ in the bytes of
 * digit_mask (bit d: byte d of the little-endian residue): out[0] 8-bit passes over a column (popcount(digit_mask); the columns
 * follow each other on the stream, so there are no passes over the column number), out[1] kernels of the call (the keys; per
 * column one gather per 32-bit word with set bits, three per pass, the final gather), out[2] tiles of a pass, out[3] bytes of
 * ctx-owned memory */
int msm_amd_test_fr_sort_plan(size_t n, size_t n_vec, uint32_t digit_mask, uint64_t out[4]);

/* A lookup handle over the SORTED table: the table is sorted by the kernels of msm_amd_fr_sort straight into the handle's
 * image, the insert pass of msm_amd_fr_lookup_build* then indexes the sorted rows, and the handle is marked sorted
 * (msm_amd_fr_lookup_sorted: *sorted = 1, 0 for a handle of the plain builds).  Row k of such a handle is sorted position k.
 * perm_out (optional, n_rows words in `mem` space, device: 4-byte aligned, not overlapping the table) maps position k back
 * to the caller's row: the stable sort permutation of the table.  Every call that takes a handle accepts this one unchanged;
 * msm_amd_fr_lookup_multiplicities* on it credits POSITIONS, and because the sort is stable the representative (the first
 * position of a run of equal values) is the image of the plain handle's representative (the smallest row):
 * m_sorted[k] == m_plain[perm[k]].  Limits, lifetime, errors and misuse are those of msm_amd_fr_lookup_build*; an unknown
 * mem is MSM_AMD_INPUT_ERROR.  The build has two bounded waits: the digit mask of the sort, then the statistics. */
int msm_amd_fr_lookup_build_sorted(msm_amd_ctx* ctx, int mem, int scalar_layout, const void* table, size_t n_rows,
                                   uint32_t* perm_out, msm_amd_fr_lookup** out, float* kernel_ms);
int msm_amd_fr_lookup_sorted(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int* sorted);
/* Test aid: the device address of a handle's image (msm_amd_fr_lookup_info gives its size), so that a test can hand a call
 * a buffer that overlaps it and see the call refused.  The image belongs to the handle: never write to it. */
int msm_amd_test_fr_lookup_image(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, void** image);

/* A', S' of msm_amd_fr_lookup_permute in a chosen arrangement, on host or on device buffers.
 * MSM_AMD_PERMUTE_ROWS works on any handle and returns exactly the bytes of msm_amd_fr_lookup_permute (over a sorted handle
 * "row" reads "sorted position").
 * MSM_AMD_PERMUTE_HALO2 needs a handle of msm_amd_fr_lookup_build_sorted (otherwise MSM_AMD_INPUT_ERROR before any launch) and
 * follows upstream's permute_expression_pair (halo2_proofs, plonk/lookup/prover.rs) with its tie-breaks: A' is the input column
 * sorted ascending by value; at position 0 and at every position where A' differs from its predecessor S' takes A''s value,
 * and one instance of that value leaves the table multiset; the leftover table values, ascending and duplicates included,
 * fill the remaining positions from the LAST one downwards (repeated_input_rows.pop()).  A = [2,2,1,2,5], S = [5,1,2,7,1]
 * give A' = [1,2,2,2,5], S' = [1,2,7,1,5] (tests/golden/permute_halo2_known.json).  halo2 is not on the build machine: the
 * bytes follow upstream's algorithm AS WRITTEN THERE and are NOT confirmed against a halo2 build.
 * How: over a sorted handle the row-order pipeline already yields halo2's A' and halo2's heads; only the gaps are filled from
 * the other end of the unused rows (fr_permute.hip.h).  A' and the heads of the two arrangements agree on a sorted handle.
 * mem.  MSM_AMD_MEM_HOST: as msm_amd_fr_lookup_permute.  MSM_AMD_MEM_DEVICE: in, a_out, s_out are device pointers to 16-byte
 * aligned records, none of which may overlap the handle's image; a_out may be `in`; report is HOST memory; the fill kernel
 * reads the miss counter on the device, so a miss leaves both outputs untouched here too.
 * Everything else -- the report, a miss, s_out needs n == n_rows, n == 0, the limits, the other argument errors, the two
 * environment knobs -- is as for msm_amd_fr_lookup_permute; an unknown mem or arrangement is MSM_AMD_INPUT_ERROR.  The twin
 * takes the table itself and, for MSM_AMD_PERMUTE_HALO2, sorts it first. */
enum { MSM_AMD_PERMUTE_ROWS = 0, MSM_AMD_PERMUTE_HALO2 = 1 };
int msm_amd_fr_lookup_permute_as(msm_amd_ctx* ctx, const msm_amd_fr_lookup* lookup, int mem, int scalar_layout,
                                 int arrangement, const void* in, size_t n, size_t n_vec, void* a_out, void* s_out,
                                 uint64_t report[4] /* HOST memory */, float* kernel_ms);
int msm_amd_host_fr_lookup_permute_as(int scalar_layout, int arrangement, const void* table, size_t n_rows,
                                      const void* in, size_t n, size_t n_vec, int threads, void* a_out, void* s_out,
                                      uint64_t report[4]);

/* ---- pairings ---------------------------------------------------------------------------------
 * The optimal ate pairing of BN254, e: G1 x G2 -> GT, in groups of pairs: the one operation that connects the two groups
 * the calls above handle (an SRS consistency check, a Groth16 or KZG verification where the proof was made, the inner
 * pairing product of proof aggregation).
 * Definition.  x = 4965661367192848881, p = 36x^4 + 36x^3 + 24x^2 + 6x + 1, r = 36x^4 + 36x^3 + 18x^2 + 6x + 1.
 *   Fq2 = Fq[u] / (u^2 + 1), xi = 9 + u, Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v); the twist y^2 = x^3 + 3 / xi.
 *   e(P, Q) = f^((p^12 - 1) / r) with f = f_{6x+2,Q}(P) l_{T,pi(Q)}(P) l_{T+pi(Q),-pi^2(Q)}(P), pi the p-power Frobenius
 *   on the twist, lines evaluated at P through the untwist.  The exponent is exactly (p^12 - 1) / r, no multiple of it.
 *   A pair in which P or Q is the identity contributes 1.
 * GT record: MSM_AMD_GT_BYTES = 384, twelve Fq of 32 bytes, little-endian, canonical (< p), in the order c0.c0.c0,
 *   c0.c0.c1, c0.c1.c0, c0.c1.c1, c0.c2.c0, c0.c2.c1, c1.c0.c0, ..., c1.c2.c1 (the field order of the Fq12 structs of
 *   arkworks and halo2curves).  MSM_AMD_GT_MONT_LE: Montgomery, R = 2^256; MSM_AMD_GT_CANON_LE: plain residues.
 *   Byte equality with either library is NOT confirmed (tests/golden/pairing_known.json).
 * Groups.  Group g is the product over the pairs g group_size .. (g + 1) group_size - 1 of the two point arrays;
 *   out_gt holds n_groups records.  group_size = 1: independent pairings; n_groups = 1: one pairing product;
 *   group_size = 0: every group is the unit.  is_one (optional): one byte per group, 1 iff its result is the unit --
 *   the pairing check.
 * flags.  MSM_AMD_PAIRING_MILLER_ONLY writes the group's Miller product instead of the pairing, for callers that
 *   multiply further before ONE msm_amd_final_exponentiation.  Such a record is a REPRESENTATIVE: a Miller value is
 *   defined only up to factors that the final exponentiation removes, and only its final exponentiation is
 *   specified (the device and the host twin do write the same bytes).  is_one must be NULL under this flag.
 * Points: the four G1 host layouts and the two G2 host layouts; the _device forms also take MSM_AMD_POINT_PREPARED /
 *   MSM_AMD_G2_POINT_PREPARED records.  Table handles are refused.  Points are NOT validated: run the point checks of
 *   both groups first (MSM_AMD_CHECK_CURVE, and MSM_AMD_CHECK_SUBGROUP for G2) on input that is not trusted.  For a
 *   point off its curve or outside the r-torsion the result is unspecified, but the call returns and reads and
 *   writes nothing out of bounds: the line formulas are projective and division-free, so even T = +-Q in an addition
 *   step only yields zeros.
 * Status.  MSM_AMD_INPUT_ERROR, output untouched: a null pointer with work to do; n_groups * group_size >= 2^32; an
 *   unknown or refused layout; unknown flags; is_one with MILLER_ONLY.  n_groups == 0 returns MSM_AMD_OK.
 * Where the final exponentiation runs.  One lane per group is slow for few groups: in the host-buffer form, below
 *   MSM_AMD_PAIRING_DEVICE_FINAL_FROM groups (environment, read at every call; default 768, the measured crossover on one MI355X
 *   against sixteen host threads) the Miller products come back and the host twin finishes them; the bytes are the same.  The _device
 *   forms always finish on the device.  MSM_AMD_PAIRING_PAIRS_PER_LANE (1, 2, 4; default 1) sets how many pairs one lane takes,
 *   MSM_AMD_PAIRING_F_IN_LDS (0, 1) where the Miller kernel keeps its running f. */
enum { MSM_AMD_GT_MONT_LE = 0, MSM_AMD_GT_CANON_LE = 1 };
enum { MSM_AMD_GT_BYTES = 384 };
enum { MSM_AMD_PAIRING_MILLER_ONLY = 1 };
int msm_amd_pairing_product(msm_amd_ctx* ctx, int point_layout, int g2_point_layout, const void* g1_points,
                            const void* g2_points, size_t n_groups, size_t group_size, uint32_t flags, int gt_layout,
                            void* out_gt, uint8_t* is_one);
int msm_amd_pairing_product_device(msm_amd_ctx* ctx, int point_layout, int g2_point_layout, const void* d_g1_points,
                                   const void* d_g2_points, size_t n_groups, size_t group_size, uint32_t flags,
                                   int gt_layout, void* d_out_gt, uint8_t* d_is_one, float* kernel_ms);
int msm_amd_host_pairing_product(int point_layout, int g2_point_layout, const void* g1_points, const void* g2_points,
                                 size_t n_groups, size_t group_size, uint32_t flags, int gt_layout, void* out_gt,
                                 uint8_t* is_one, int threads);
/* out[i] = in[i]^((p^12 - 1) / r) for n GT records of gt_layout (any 256-bit field is taken mod p); out may be in;
 * is_one optional.  The host-buffer form follows the placement rule above with n in the place of the group count. */
int msm_amd_final_exponentiation(msm_amd_ctx* ctx, int gt_layout, const void* in, size_t n, void* out, uint8_t* is_one);
int msm_amd_final_exponentiation_device(msm_amd_ctx* ctx, int gt_layout, const void* d_in, size_t n, void* d_out,
                                        uint8_t* d_is_one, float* kernel_ms);
int msm_amd_host_final_exponentiation(int gt_layout, const void* in, size_t n, void* out, uint8_t* is_one, int threads);
/* Test aid (no ctx): the plan of a pairing product.  pairs_per_lane: 0 for the default rule, else the knob's value;
 * device_final_from: the group count from which the device finishes, UINT64_MAX for the library's own default.  out: [0] pairs per lane, [1] lanes per group
 * (ceil(group_size / [0]), at least 1), [2] fold levels (each multiplies four partials per lane), [3] 1 if the final
 * exponentiation runs on the device. */
int msm_amd_test_pairing_plan(size_t n_groups, size_t group_size, uint32_t pairs_per_lane, uint64_t device_final_from,
                              uint32_t out[4]);
/* Test aid: one op of the device's Fq12 arithmetic (bn254_fq12_29.hip.h) on raw 29-bit limbs, one element per call.
 * a, b, out: MSM_AMD_FQ12_WORDS u32 each; an Fq12 in the order of the GT record, 18 words per Fq2 (c0 limbs 0..8, c1
 * limbs 0..8); an Fq6 in the first 54 words.  Operands obey the bounds contract of that header (normalised limbs,
 * at most 4 p per component; line coefficients below 8 p).  LINE_MUL: b = l0, l1, l3.  DOUBLE_STEP: a = T (X, Y, Z),
 * b = x_P, y_P (9 words each); out = T', then l0, l1, l3.  ADD_STEP: the same with Q (x, y) behind T in a.
 * FINAL_EXP: fq12_final_exp on the raw element a (the path of the fused product kernel), raw element out; a = 0 gives
 * an element, not a fault.  An unknown op is refused.
 * The *_ops forms run count records (count * MSM_AMD_FQ12_WORDS words each way, at most 2^20 records) in one launch, one
 * lane per record; count = 0 returns MSM_AMD_OK and touches nothing.  The one-record calls are the count = 1 case. */
enum {
  MSM_AMD_FQ12_OP_FQ6_MUL = 0, MSM_AMD_FQ12_OP_MUL = 1, MSM_AMD_FQ12_OP_SQR = 2, MSM_AMD_FQ12_OP_CYCLO_SQR = 3,
  MSM_AMD_FQ12_OP_LINE_MUL = 4, MSM_AMD_FQ12_OP_FROB1 = 5, MSM_AMD_FQ12_OP_FROB2 = 6, MSM_AMD_FQ12_OP_FROB3 = 7,
  MSM_AMD_FQ12_OP_CONJ = 8, MSM_AMD_FQ12_OP_INV = 9, MSM_AMD_FQ12_OP_POW_X = 10, MSM_AMD_FQ12_OP_DOUBLE_STEP = 11,
  MSM_AMD_FQ12_OP_ADD_STEP = 12, MSM_AMD_FQ12_OP_FINAL_EXP = 13
};
enum { MSM_AMD_FQ12_WORDS = 108 };
int msm_amd_test_fq12_op(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out);
int msm_amd_test_fq12_op_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out);
int msm_amd_test_fq12_ops(msm_amd_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);
int msm_amd_test_fq12_ops_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count);

/* ---- introspection --------------------------------------------------------------------------- */
int msm_amd_last_timings(const msm_amd_ctx* ctx, msm_amd_timings* out);
/* Algorithmic HBM bytes of one MSM: whole pipeline and accumulation only. */
uint64_t msm_amd_algorithmic_bytes(size_t n, uint32_t window_size, int accumulate_only);
const char* msm_amd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSM_AMD_H */
