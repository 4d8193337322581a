// Kernels of the lookup tables over BN254 Fr (fr_lookup.hip.h):
//   fr_lookup_rows_kernel    one lane per row: the caller's record -> the reduced Montgomery residue in the handle's image.
//   fr_lookup_insert_kernel  one lane per row: fr_lookup_insert with vector atomics on the slot words (a relaxed device-scope
//                            load, compare-and-swap on an empty slot, atomic minimum on an equal occupant).  The wave folds
//                            its claimed slots, its longest probe and its error flag, one lane adds them to the statistics.
//   fr_lookup_probe_kernel   one lane per input: fr_lookup_find with plain loads (the index was finished by an earlier
//                            launch), the row index to idx_out, the misses of the wave counted by one lane (the lowest
//                            missing lane holds the smallest flat index of the wave), and the hit counted in the row's
//                            32-bit counter: <kLookupCountLane> one atomic per lane, <kLookupCountWave> one atomic per
//                            distinct row of the wave -- the lanes that found the same row elect the lowest of them, who
//                            adds their number; the loop runs once per distinct row, at most 64 times, and is uniform;
//                            <kLookupCountBlock> the same in workgroups of 16 waves, each wave holding its largest group
//                            back: the held groups meet in LDS behind one barrier and leave as one atomic per distinct row
//                            (a column that is half zeros sends one add per 1024 inputs to the counter of 0, not 16).
//                            <.., COLS> (msm_amd_fr_lookup_permute*, k_permute.hip): every column of inputs counts in
//                            counters of its own.
//   fr_lookup_finish_kernel  one lane per row: the counter -> m_out[j] as a record of the caller's layout; rows hit and the
//                            largest counter folded per wave.  STRICT: the lanes read the miss counter of the probe launch
//                            and store nothing if it is not zero.
// Phases are ordered by launch order on one stream.  Every probe loop ends after `capacity` slots.
#include "launch_fr.h"

namespace msm_amd {

namespace {

__device__ __forceinline__ u256 load_rec(const uint32_t* rec) {
  const uint4 a = ((const uint4*)rec)[0], b = ((const uint4*)rec)[1];
  u256 x;
  x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w, x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
  return x;
}
__device__ __forceinline__ void store_rec(uint32_t* rec, const u256& x) {
  ((uint4*)rec)[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  ((uint4*)rec)[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// the index while it is being built
struct BuildMem {
  const uint32_t* rows;
  uint32_t* slots;
  __device__ uint32_t load(uint32_t at) { return __hip_atomic_load(slots + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ uint32_t cas(uint32_t at, uint32_t expect, uint32_t value) { return atomicCAS(slots + at, expect, value); }
  __device__ void lower(uint32_t at, uint32_t value) { atomicMin(slots + at, value); }
  __device__ u256 row(uint32_t i) { return load_rec(rows + (uint64_t)i * 8); }
};
// a finished index
struct ProbeMem {
  const uint32_t* rows;
  const uint32_t* slots;
  __device__ uint32_t load(uint32_t at) { return slots[at]; }
  __device__ u256 row(uint32_t i) { return load_rec(rows + (uint64_t)i * 8); }
};

__global__ void __launch_bounds__(kLookupThreads) fr_lookup_rows_kernel(int layout, const uint32_t* table, uint64_t n_rows,
                                                                         uint32_t* rows) {
  const uint64_t i = (uint64_t)blockIdx.x * kLookupThreads + threadIdx.x;
  if (i >= n_rows) return;
  store_rec(rows + i * 8, fr_load(layout, load_rec(table + i * 8)));
}

__global__ void __launch_bounds__(kLookupThreads) fr_lookup_insert_kernel(FrLookupPlan plan, const uint32_t* rows, uint64_t n_rows,
                                                                           uint32_t* slots, uint32_t* stats) {
  const uint64_t i = (uint64_t)blockIdx.x * kLookupThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  uint32_t steps = 0;
  bool claimed = false, failed = false;
  if (i < n_rows) {
    BuildMem mem{rows, slots};
    steps = fr_lookup_insert(plan, mem, (uint32_t)i, load_rec(rows + i * 8), &claimed);
    failed = steps == 0;
  }
  const uint32_t took = (uint32_t)__popcll(__ballot(claimed));
  const bool any_failed = __ballot(failed) != 0;
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)steps, (int)d);
    steps = other > steps ? other : steps;
  }
  if (lane != 0) return;
  if (took) atomicAdd(stats + kLookupDistinct, took);
  if (steps) atomicMax(stats + kLookupLongest, steps);
  if (any_failed) atomicMax(stats + kLookupError, 1u);
}

struct FrLookupProbeArgs {
  FrLookupPlan plan;
  const uint32_t* rows;
  const uint32_t* slots;
  const uint32_t* in;
  uint64_t total;
  uint32_t* idx_out;              // optional
  uint32_t* counters;             // n_rows; COLS: n_rows for each column
  unsigned long long* report;     // kLookupReportWords
  int layout;
  uint32_t col_n, n_rows;         // COLS: inputs per column, counters per column
};

// COLS (msm_amd_fr_lookup_permute*): input i of column i / col_n counts in that column's counters; a wave or a workgroup
// that straddles a column boundary groups by the flat counter index, which is below 2^32
template <int FORM, bool COLS>
__global__ void __launch_bounds__(FORM == kLookupCountBlock ? kLookupBlockThreads : kLookupThreads)
    fr_lookup_probe_kernel(FrLookupProbeArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  const bool active = i < a.total;
  uint32_t idx = kLookupEmpty;
  bool exhausted = false;
  if (active) {
    ProbeMem mem{a.rows, a.slots};
    idx = fr_lookup_find(a.plan, mem, fr_load(a.layout, load_rec(a.in + i * 8)), &exhausted);
    if (a.idx_out) a.idx_out[i] = idx;
  }
  const bool hit = active && idx != kLookupEmpty;
  const unsigned long long missing = __ballot(active && !hit);
  if (missing && lane == (uint32_t)__ffsll(missing) - 1u) {
    atomicAdd(a.report + kLookupMissing, (unsigned long long)__popcll(missing));
    atomicMin(a.report + kLookupFirstMissing, (unsigned long long)i);
  }
  if (exhausted) atomicMax(a.report + kLookupReportError, 1ull);
  if (COLS && hit) idx += (uint32_t)(i / a.col_n) * a.n_rows;
  if (FORM == kLookupCountLane) {
    if (hit) atomicAdd(a.counters + idx, 1u);
    return;
  }
  // every value below is uniform over the wave; the largest group of the wave is held back for the workgroup (kLookupCountBlock)
  uint32_t held_key = 0, held = 0;
  unsigned long long todo = __ballot(hit);
  NTT_NO_UNROLL while (todo) {
    const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;
    uint32_t key = (uint32_t)__shfl((int)idx, (int)leader);
    const unsigned long long same = __ballot(hit && idx == key);
    uint32_t count = (uint32_t)__popcll(same);
    todo &= ~same;
    if (FORM == kLookupCountBlock && count > held) {
      const uint32_t k = held_key, c = held;
      held_key = key, held = count;
      key = k, count = c;
    }
    if (count && lane == leader) atomicAdd(a.counters + key, count);
  }
  if (FORM != kLookupCountBlock) return;
  // the held groups of the workgroup's waves: equal rows are added up, one atomic per distinct row
  __shared__ uint32_t wave_key[kLookupBlockThreads / kFrWave], wave_count[kLookupBlockThreads / kFrWave];
  const uint32_t wave = threadIdx.x / kFrWave, waves = blockDim.x / kFrWave;
  if (lane == 0) wave_key[wave] = held_key, wave_count[wave] = held;
  __syncthreads();
  if (threadIdx.x >= waves || wave_count[threadIdx.x] == 0) return;
  const uint32_t mine = wave_key[threadIdx.x];
  uint32_t sum = 0;
  NTT_NO_UNROLL for (uint32_t w = 0; w < waves; ++w) {
    if (wave_count[w] == 0 || wave_key[w] != mine) continue;
    if (w < threadIdx.x) return;   // an earlier wave held the same row: its lane adds for both
    sum += wave_count[w];
  }
  atomicAdd(a.counters + mine, sum);
}

__global__ void __launch_bounds__(kLookupThreads) fr_lookup_finish_kernel(int layout, int on_missing, const uint32_t* counters,
                                                                           uint64_t n_rows, unsigned long long* report,
                                                                           uint32_t* m_out) {
  const uint64_t j = (uint64_t)blockIdx.x * kLookupThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kFrWave - 1);
  const uint32_t c = j < n_rows ? counters[j] : 0u;
  const uint32_t rows_hit = (uint32_t)__popcll(__ballot(c != 0));
  uint32_t most = c;
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)most, (int)d);
    most = other > most ? other : most;
  }
  if (lane == 0 && rows_hit) {
    atomicAdd(report + kLookupRowsHit, (unsigned long long)rows_hit);
    atomicMax(report + kLookupMaxMult, (unsigned long long)most);
  }
  if (j >= n_rows) return;
  // the miss counter is complete: the probe launch came before this one
  if (on_missing == kLookupStrict && report[kLookupMissing] != 0) return;
  store_rec(m_out + j * 8, fr_store(layout, fr_lookup_count(c)));
}

uint32_t blocks_of(uint64_t items) { return (uint32_t)((items + kLookupThreads - 1) / kLookupThreads); }

template <bool COLS>
void launch_probe(hipStream_t st, int count_form, const FrLookupProbeArgs& a) {
  if (count_form == kLookupCountLane)
    hipLaunchKernelGGL((fr_lookup_probe_kernel<kLookupCountLane, COLS>), dim3(blocks_of(a.total)), dim3(kLookupThreads), 0, st, a);
  else if (count_form == kLookupCountWave)
    hipLaunchKernelGGL((fr_lookup_probe_kernel<kLookupCountWave, COLS>), dim3(blocks_of(a.total)), dim3(kLookupThreads), 0, st, a);
  else
    hipLaunchKernelGGL((fr_lookup_probe_kernel<kLookupCountBlock, COLS>),
                       dim3((uint32_t)((a.total + kLookupBlockThreads - 1) / kLookupBlockThreads)), dim3(kLookupBlockThreads), 0,
                       st, a);
}

}  // namespace

void launch_fr_lookup_build(hipStream_t st, const FrLookupPlan& plan, uint64_t n_rows, int layout, const void* d_table,
                            void* image) {
  uint8_t* base = (uint8_t*)image;
  uint32_t* rows = (uint32_t*)(base + plan.rows_off);
  uint32_t* slots = (uint32_t*)(base + plan.slots_off);
  uint32_t* stats = (uint32_t*)(base + plan.stats_off);
  (void)hipMemsetAsync(slots, 0xFF, plan.capacity * 4, st);
  (void)hipMemsetAsync(stats, 0, kLookupStatWords * 4, st);
  if (d_table)
    hipLaunchKernelGGL(fr_lookup_rows_kernel, dim3(blocks_of(n_rows)), dim3(kLookupThreads), 0, st, layout,
                       (const uint32_t*)d_table, n_rows, rows);
  hipLaunchKernelGGL(fr_lookup_insert_kernel, dim3(blocks_of(n_rows)), dim3(kLookupThreads), 0, st, plan, (const uint32_t*)rows,
                     n_rows, slots, stats);
}

void launch_fr_lookup_probe(hipStream_t st, const FrLookupLaunch& c, uint64_t col_n, uint32_t* counters,
                            unsigned long long* report) {
  const uint8_t* image = (const uint8_t*)c.image;
  FrLookupProbeArgs a{};
  a.plan = c.plan;
  a.rows = (const uint32_t*)(image + c.plan.rows_off), a.slots = (const uint32_t*)(image + c.plan.slots_off);
  a.in = (const uint32_t*)c.in, a.total = c.total, a.idx_out = c.idx_out;
  a.counters = counters, a.report = report, a.layout = c.layout;
  a.col_n = (uint32_t)col_n, a.n_rows = (uint32_t)c.n_rows;
  if (col_n) launch_probe<true>(st, c.count_form, a);
  else launch_probe<false>(st, c.count_form, a);
}

uint32_t launch_fr_lookup_multiplicities(hipStream_t st, const FrLookupLaunch& c) {
  uint8_t* work = (uint8_t*)c.work;
  unsigned long long* report = (unsigned long long*)(work + c.at.report_off);
  (void)hipMemsetAsync(work, 0, c.at.idx_off, st);
  (void)hipMemsetAsync(report + kLookupFirstMissing, 0xFF, 8, st);
  uint32_t launches = 1;
  if (c.total) {
    launch_fr_lookup_probe(st, c, 0, (uint32_t*)work, report);
    ++launches;
  }
  hipLaunchKernelGGL(fr_lookup_finish_kernel, dim3(blocks_of(c.n_rows)), dim3(kLookupThreads), 0, st, c.layout, c.on_missing,
                     (const uint32_t*)work, c.n_rows, report, (uint32_t*)c.m_out);
  return launches;
}

}  // namespace msm_amd
