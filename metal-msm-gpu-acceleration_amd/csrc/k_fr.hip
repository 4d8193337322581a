// Kernels over vectors of BN254 Fr (fr_vec.hip.h):
//   fr_map_kernel<OP>      one lane per record, consecutive lanes on consecutive records: load (to_mont for CANON_LE), the
//                          op, store (from_mont for CANON_LE).  k arrives by value.
//   (the two tile kernels are templates on the monoid: <false> the products, <true> the sums of msm_amd_fr_prefix_sum*,
//   where "product" below reads "sum" and "one" reads "zero"; fr_map_kernel<kFrShift> is a + k)
//   fr_tile_reduce_kernel  one wave per tile: every lane multiplies the records lane, lane + 64, ... of the tile, six
//                          shuffle steps fold the 64 lane products; the inversion's form reads a zero as one and counts it.
//   fr_tile_scan_kernel    one wave per tile: the tile goes to LDS at unit stride, lane t owns the 2^(T-6) consecutive
//                          records t 2^(T-6) ..: its product (lane 0 starts from the tile's carry), six shuffle steps for
//                          the inclusive scan of the 64 lane products, a second walk that writes the running products
//                          back to LDS, and the tile leaves at unit stride.
//   fr_inv_apply_kernel    one wave per tile, two LDS images (the records, and the running product before each record of
//                          a lane): c = T^-1 P_(b-1) S_(b+1) inverts the tile's product, the prefix and suffix scans of
//                          the lane products turn it into the inverse of each lane's product, and the backward sweep of
//                          the classic batch inversion runs inside the lane.
//   fr_poly_reduce_kernel  one wave per tile, no LDS: the tile's value H_b = sum_m c_(b 2^T + m) z^m.  Lane l runs Horner in
//                          z^64 over the records l, l + 64, ..., six xor-shuffle steps v_l += z^(2^s) v_(l xor 2^s) fold
//                          the lanes; a partial tile reads as padded with zeros.
//   fr_poly_scan_kernel    one wave per tile: s_i = sum_(j >= i) c_j z^(j - i).  The tile goes to LDS at unit stride, lane
//                          t walks its records backwards, acc = acc z + c (the lane of a full tile's last record starts
//                          from the tile's carry, s at the first record of the next tile), six shuffle steps with the
//                          uniform multipliers z^(per 2^s) for the suffix scan of the lane values, a second backward
//                          walk that writes s_(i+1) (the division) or s_i (the upper levels) to LDS, and the tile leaves
//                          at unit stride.  Tiles start at index 0 of a vector, so that only the highest tile is partial
//                          and its carry is zero: every multiplier is uniform.
//   fr_poly_points_reduce_kernel<K>, fr_poly_points_scan_kernel<K>  the two kernels above at K points side by side (fr_vec.hip.h):
//                          a record is loaded (reduce) or read from the LDS image (scan) once and feeds K running values,
//                          which live in registers -- K is a template argument and every loop over the points is unrolled;
//                          the K chains of products are independent, so one wave has K of them in flight where the
//                          single-point kernels have one.  The scan of level 0 writes sum_j w_j s^(j)_(i+1) per record as
//                          sum_(j < K-1) w_j (s^(j) - s^(K-1)).  blockIdx.y picks the block's group of K points: one group
//                          at level 0, and K = 1 with one block row per point at the levels above, where point j reads and
//                          writes its own copy of the totals.  The powers and weights of all points come by value and
//                          are read at wave-uniform offsets.
//   fr_lincomb_kernel      one lane per index i: Horner in k over a_v[i], v from the last vector down.
//   fr_mat_lane_kernel     y = M x, rows of at most LONG entries (fr_mat.hip.h): one lane per row, consecutive lanes on
//                          consecutive rows; per entry one 8-byte (column, id) load, the dictionary record and the gathered
//                          x record (two dwordx4 each), one product, one addition.  A lane of a longer row stores nothing.
//                          <SIGNS>: an entry whose value is 1 or r - 1 is added or subtracted without a product.
//   fr_mat_wave_kernel     one wave per segment of a longer row: lane l takes the entries l, l + 64, ..., six xor-shuffle
//                          additions fold the lanes, lane 0 stores y[row], or the raw partial sum of a split row.
//   fr_mat_fold_kernel     one wave per split row: the sum of its partials, the same fold, y[row].
//   fr_sumcheck_round_kernel<FORM, K>  (fr_mle.hip.h) one wave per chunk of 2^C pairs: lane l takes the pairs l, l + 64, ... of
//                          the chunk (HIGH: both records at unit stride across the wave; LOW: the two records of a pair are 64
//                          contiguous bytes), d + 1 sums per lane in registers, six xor-shuffle additions each, lane 0 stores
//                          d + 1 raw partial records.
//   fr_sumcheck_terms_kernel<D>  the same wave per chunk over a caller's sum of products of degree D (FrTermSums): the terms
//                          and their factors in runtime loops of wave-uniform trip counts, a pair loaded per use.
//   fr_gate_kernel         (fr_gate.hip.h) one lane per row of a sum of products of rotated columns, consecutive lanes on
//                          consecutive rows: every rotated read is coalesced except in the one workgroup where it wraps;
//                          the terms and their factors in runtime loops of wave-uniform trip counts, a record loaded per
//                          use; the image by value, the periodic scale from a table of at most 256 raw records.
//   fr_mle_fold_kernel     one wave per 2^10 partials of one t: their sum, the same fold.
//   fr_mle_eval_kernel<P>  one wave per tile of 2^c records: lane l folds the records l, l + 64, ... (a tree in registers
//                          over the tile's upper variables), six xor-shuffle steps fold the variables of the lane index,
//                          lane 0 stores the tile's record.
//   fr_mle_bind_kernel<K>  one lane per output: a tree over its 2^K records (HIGH: n / 2^K apart, unit stride across the
//                          lanes; LOW: 2^K consecutive records).
//   fr_eq_table_kernel<S>  one lane per 2^S outputs: the product of the factors of the index bits below, then S doublings;
//                          the 2 m factors come by value.
//   fr_poseidon_kernel<T, KIND>  (fr_poseidon.hip.h) one lane per permutation of a state of T records (KIND: the bare
//                          permutation, or the hash of T - 1 records under a tag); the workgroup stages the constants image
//                          in LDS once and every lane reads it at wave-uniform addresses; nothing per lane comes from memory
//                          between the load of its inputs and the store of its outputs.
//   fr_poseidon_tail_kernel<T>  the last levels of a Merkle tree in ONE workgroup: a level, a barrier, the next level from the
//                          nodes just stored to the tree.
//   fr_merkle_paths_kernel one lane per sibling record of an authentication path: a gather over the leaves and the tree.
// Phases are ordered by launch order on one stream only; no kernel reads what another workgroup of its launch wrote.
// LDS images are eight word planes; slot m sits at m + (m >> log2(records per lane)), so that the unit-stride accesses
// and the walks of the lanes (stride = records per lane) are both free of bank conflicts, bar one 2-way per access.
// No scratch, no register array indexed at run time (`make resource-usage`); the walks are not unrolled.
#include "launch_fr.h"

namespace msm_amd {

namespace {

struct FrTileArgs {
  const uint32_t* src;
  uint32_t* dst;               // scan
  const uint32_t* carry;       // scan: one raw record per tile, the product before it; null: one
  uint32_t* totals;            // reduce: one raw record per tile
  unsigned long long* zeros;   // reduce with zero_one: the count
  uint64_t len, tiles;         // records and tiles per vector
  uint32_t tile_log;
  int layout, mode, reverse, zero_one;
};

struct FrInvArgs {
  const uint32_t* src;
  uint32_t* dst;
  const uint32_t* P;
  const uint32_t* S;
  uint64_t len, tiles;
  uint32_t tile_log;
  int layout;
  u256 t_inv;
};

// The powers of a level's point z come by value: no table in memory, no power computed on the device
struct FrPolyArgs {
  const uint32_t* src;
  uint32_t* dst;               // scan
  const uint32_t* carry;       // scan: the level above, s of tile b + 1 is the carry of tile b; null: every carry is zero
  uint32_t* totals;            // reduce: one raw record per tile; scan: s_0 of every tile, raw (optional)
  uint64_t len, tiles;         // records and tiles per vector
  uint32_t tile_log;
  int layout, shift;           // shift: slot i takes s_(i+1), the quotient by X - z
  u256 z;                      // the point of the level
  u256 step[7];                // reduce: z^(2^s), s < 6, and z^64; scan: z^(per 2^s), s < 6
};

// An LDS image of a tile: eight planes of 2^T + 64 words, sized at the launch (fr_image_bytes) so that a smaller tile
// lets more waves share a CU
struct Image {
  uint32_t* lds;
  uint32_t plane, per_log;
};
__host__ __device__ constexpr uint32_t fr_image_bytes(uint32_t tile_log) { return 8u * ((1u << tile_log) + kFrWave) * 4u; }
__device__ __forceinline__ Image image(uint32_t* lds, uint32_t tile_log) {
  return Image{lds, (1u << tile_log) + kFrWave, tile_log > 6u ? tile_log - 6u : 0u};
}
__device__ __forceinline__ u256 lds_get(const Image& im, uint32_t m) {
  const uint32_t p = m + (m >> im.per_log);
  u256 x;
  MSM_UNROLL for (int w = 0; w < 8; ++w) x.v[w] = im.lds[w * im.plane + p];
  return x;
}
__device__ __forceinline__ void lds_put(const Image& im, uint32_t m, const u256& x) {
  const uint32_t p = m + (m >> im.per_log);
  MSM_UNROLL for (int w = 0; w < 8; ++w) im.lds[w * im.plane + p] = x.v[w];
}

// 32-byte records of 16-byte aligned buffers move as two dwordx4
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

__device__ __forceinline__ u256 wave_up(const u256& x, uint32_t d) {
  u256 r;
  MSM_UNROLL for (int w = 0; w < 8; ++w) r.v[w] = __shfl_up(x.v[w], d);
  return r;
}
__device__ __forceinline__ u256 wave_down(const u256& x, uint32_t d) {
  u256 r;
  MSM_UNROLL for (int w = 0; w < 8; ++w) r.v[w] = __shfl_down(x.v[w], d);
  return r;
}
__device__ __forceinline__ u256 wave_xor(const u256& x, uint32_t d) {
  u256 r;
  MSM_UNROLL for (int w = 0; w < 8; ++w) r.v[w] = __shfl_xor(x.v[w], (int)d);
  return r;
}

// The tile of a workgroup: vector v, first index and record count inside the vector
struct TilePlace {
  uint64_t base, first;
  uint32_t cnt;
};
__device__ __forceinline__ TilePlace tile_place(uint64_t b, uint64_t len, uint64_t tiles, uint32_t tile_log) {
  TilePlace t;
  const uint64_t v = b / tiles;
  t.base = v * len;
  t.first = (b - v * tiles) << tile_log;
  const uint64_t left = len - t.first;
  t.cnt = left < ((uint64_t)1 << tile_log) ? (uint32_t)left : (1u << tile_log);
  return t;
}
// slot m of the tile -> record of the buffer (reverse: the vector is walked from its last record down)
__device__ __forceinline__ uint64_t tile_record(const TilePlace& t, uint64_t len, int reverse, uint32_t m) {
  const uint64_t i = t.first + m;
  return t.base + (reverse ? len - 1 - i : i);
}

template <int OP>
__global__ void __launch_bounds__(kFrMapThreads) fr_map_kernel(int layout, u256 k, const uint32_t* A, const uint32_t* B,
                                                                const uint32_t* C, uint64_t n, uint32_t* out) {
  constexpr unsigned reads = fr_op_reads(OP);
  const uint64_t i = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (i >= n) return;
  const u256 a = fr_load(layout, load_rec(A + i * 8));
  u256 b = a, c = a;
  if (reads & kFrReadsB) b = fr_load(layout, load_rec(B + i * 8));
  if (reads & kFrReadsC) c = fr_load(layout, load_rec(C + i * 8));
  store_rec(out + i * 8, fr_store(layout, fr_map_op<OP>(k, a, b, c)));
}

template <bool SUM>
__global__ void __launch_bounds__(kFrWave) fr_tile_reduce_kernel(FrTileArgs a) {
  const uint32_t lane = threadIdx.x;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  u256 acc = fr_scan_unit<SUM>();
  uint32_t zc = 0;
  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave) {
    u256 x = fr_load(a.layout, load_rec(a.src + tile_record(t, a.len, a.reverse, m) * 8));
    if (!SUM && a.zero_one) {
      const bool z = u256_is_zero(x);
      zc += z ? 1u : 0u;
      x = fr_select(z, Fr::one(), x);
    }
    acc = fr_scan_op<SUM>(acc, x);
  }
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) {
    acc = fr_scan_op<SUM>(acc, wave_xor(acc, d));
    zc += (uint32_t)__shfl_xor((int)zc, (int)d);
  }
  if (lane == 0) {
    store_rec(a.totals + (uint64_t)blockIdx.x * 8, acc);
    if (!SUM && a.zero_one && zc) atomicAdd(a.zeros, (unsigned long long)zc);
  }
}

template <bool SUM>
__global__ void __launch_bounds__(kFrWave) fr_tile_scan_kernel(FrTileArgs a) {
  extern __shared__ uint32_t fr_lds[];
  const Image lds = image(fr_lds, a.tile_log);
  const uint32_t lane = threadIdx.x;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  const uint32_t per = 1u << lds.per_log, m0 = lane << lds.per_log;

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    lds_put(lds, m, fr_load(a.layout, load_rec(a.src + tile_record(t, a.len, a.reverse, m) * 8)));
  __syncthreads();

  // the product of the lane's records; lane 0 carries the product before the tile
  const u256 unit = fr_scan_unit<SUM>();
  const u256 carry = a.carry ? load_rec(a.carry + (uint64_t)blockIdx.x * 8) : unit;
  u256 acc = fr_select(lane == 0, carry, unit);
  NTT_NO_UNROLL for (uint32_t j = 0; j < per; ++j) {
    if (m0 + j >= t.cnt) break;
    acc = fr_scan_op<SUM>(acc, lds_get(lds, m0 + j));
  }
  NTT_NO_UNROLL for (uint32_t d = 1; d < kFrWave; d <<= 1) {
    const u256 y = wave_up(acc, d);
    acc = fr_scan_op<SUM>(acc, fr_select(lane >= d, y, unit));
  }
  // the product before the lane's first record, then the running products
  u256 run = fr_select(lane == 0, carry, wave_up(acc, 1));
  NTT_NO_UNROLL for (uint32_t j = 0; j < per; ++j) {
    const uint32_t m = m0 + j;
    if (m >= t.cnt) break;
    const u256 nxt = fr_scan_op<SUM>(run, lds_get(lds, m));
    lds_put(lds, m, a.mode == kFrInclusive ? nxt : run);
    run = nxt;
  }
  __syncthreads();

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    store_rec(a.dst + tile_record(t, a.len, a.reverse, m) * 8, fr_store(a.layout, lds_get(lds, m)));
}

__global__ void __launch_bounds__(kFrWave) fr_inv_apply_kernel(FrInvArgs a) {
  extern __shared__ uint32_t fr_lds[];
  const Image lds_x = image(fr_lds, a.tile_log), lds_p = image(fr_lds + fr_image_bytes(a.tile_log) / 4u, a.tile_log);
  const uint32_t lane = threadIdx.x;
  const uint64_t b = blockIdx.x;
  const TilePlace t = tile_place(b, a.len, a.tiles, a.tile_log);
  const uint32_t per = 1u << lds_x.per_log, m0 = lane << lds_x.per_log;

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    lds_put(lds_x, m, fr_load(a.layout, load_rec(a.src + tile_record(t, a.len, 0, m) * 8)));
  __syncthreads();

  // forward: the running product before each record of the lane (zeros read as one), and the lane's product
  u256 acc = Fr::one();
  NTT_NO_UNROLL for (uint32_t j = 0; j < per; ++j) {
    const uint32_t m = m0 + j;
    if (m >= t.cnt) break;
    const u256 x = lds_get(lds_x, m);
    lds_put(lds_p, m, acc);
    acc = Fr::mul(acc, fr_select(u256_is_zero(x), Fr::one(), x));
  }
  // inclusive prefix and suffix products of the lane products
  u256 pre = acc, suf = acc;
  NTT_NO_UNROLL for (uint32_t d = 1; d < kFrWave; d <<= 1) {
    const u256 y = wave_up(pre, d), z = wave_down(suf, d);
    pre = Fr::mul(pre, fr_select(lane >= d, y, Fr::one()));
    suf = Fr::mul(suf, fr_select(lane + d < kFrWave, z, Fr::one()));
  }
  const u256 before = fr_select(lane == 0, Fr::one(), wave_up(pre, 1));
  const u256 after = fr_select(lane == kFrWave - 1, Fr::one(), wave_down(suf, 1));
  // the inverse of the tile's product, then of the lane's product
  u256 inv = a.t_inv;
  if (b > 0) inv = Fr::mul(inv, load_rec(a.P + (b - 1) * 8));
  if (b + 1 < a.tiles) inv = Fr::mul(inv, load_rec(a.S + (b + 1) * 8));
  inv = Fr::mul(Fr::mul(inv, before), after);
  // backward: inv is the inverse of the product up to and including record j
  NTT_NO_UNROLL for (uint32_t j = per; j-- != 0;) {
    const uint32_t m = m0 + j;
    if (m >= t.cnt) continue;
    const u256 x = lds_get(lds_x, m);
    const bool z = u256_is_zero(x);
    const u256 o = Fr::mul(inv, lds_get(lds_p, m));
    inv = Fr::mul(inv, fr_select(z, Fr::one(), x));
    lds_put(lds_x, m, fr_select(z, x, o));
  }
  __syncthreads();

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    store_rec(a.dst + tile_record(t, a.len, 0, m) * 8, fr_store(a.layout, lds_get(lds_x, m)));
}

__global__ void __launch_bounds__(kFrWave) fr_poly_reduce_kernel(FrPolyArgs a) {
  const uint32_t lane = threadIdx.x;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  const uint32_t* src = a.src + t.base * 8;
  u256 acc = u256_zero();
  if (lane < t.cnt) {
    // the lane's highest record first
    uint64_t i = t.first + lane + ((t.cnt - 1 - lane) & ~(kFrWave - 1));
    acc = fr_load(a.layout, load_rec(src + i * 8));
    NTT_NO_UNROLL while (i >= t.first + kFrWave) {
      i -= kFrWave;
      acc = Fr::add(Fr::mul(acc, a.step[6]), fr_load(a.layout, load_rec(src + i * 8)));
    }
  }
  NTT_NO_UNROLL for (uint32_t s = 0; s < 6; ++s) acc = Fr::add(acc, Fr::mul(a.step[s], wave_xor(acc, 1u << s)));
  if (lane == 0) store_rec(a.totals + (uint64_t)blockIdx.x * 8, acc);
}

__global__ void __launch_bounds__(kFrWave) fr_poly_scan_kernel(FrPolyArgs a) {
  extern __shared__ uint32_t fr_lds[];
  const Image lds = image(fr_lds, a.tile_log);
  const uint32_t lane = threadIdx.x;
  const uint64_t v = blockIdx.x / a.tiles, b = blockIdx.x - v * a.tiles;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  const uint32_t per = 1u << lds.per_log, m0 = lane << lds.per_log;
  const uint32_t top = ((1u << a.tile_log) >> lds.per_log) - 1u;   // the lane of a full tile's last record

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    lds_put(lds, m, fr_load(a.layout, load_rec(a.src + (t.base + t.first + m) * 8)));
  __syncthreads();

  // s at the first record of the next tile: record b + 1 of this vector in the level above
  const u256 carry = a.carry && b + 1 < a.tiles ? load_rec(a.carry + (v * a.tiles + b + 1) * 8) : u256_zero();
  u256 acc = fr_select(lane == top, carry, u256_zero());
  NTT_NO_UNROLL for (uint32_t j = per; j-- != 0;) {
    if (m0 + j >= t.cnt) continue;
    acc = Fr::add(Fr::mul(acc, a.z), lds_get(lds, m0 + j));
  }
  // the suffix scan of the lane values: acc becomes s at the lane's first record
  NTT_NO_UNROLL for (uint32_t s = 0; s < 6; ++s) {
    const uint32_t d = 1u << s;
    const u256 y = wave_down(acc, d);
    acc = Fr::add(acc, Fr::mul(a.step[s], fr_select(lane + d < kFrWave, y, u256_zero())));
  }
  if (a.totals && lane == 0) store_rec(a.totals + (uint64_t)blockIdx.x * 8, acc);
  // s behind the lane's last record, then down the lane
  u256 run = fr_select(lane == top, carry, wave_down(acc, 1));
  NTT_NO_UNROLL for (uint32_t j = per; j-- != 0;) {
    const uint32_t m = m0 + j;
    if (m >= t.cnt) continue;
    const u256 nxt = Fr::add(Fr::mul(run, a.z), lds_get(lds, m));
    lds_put(lds, m, a.shift ? run : nxt);
    run = nxt;
  }
  __syncthreads();

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    store_rec(a.dst + (t.base + t.first + m) * 8, fr_store(a.layout, lds_get(lds, m)));
}

// The points p0 .. p0 + K - 1 of the block: acc[j] belongs to point p0 + j.  blockIdx.x is the tile over all vectors.
template <int K>
__global__ void __launch_bounds__(kFrWave) fr_poly_points_reduce_kernel(FrPolyPointsArgs a) {
  const uint32_t lane = threadIdx.x, p0 = blockIdx.y * K;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  const uint32_t* src = a.src + ((uint64_t)blockIdx.y * a.src_stride + t.base) * 8;
  u256 acc[K];
  MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = u256_zero();
  if (lane < t.cnt) {
    // the lane's highest record first
    uint64_t i = t.first + lane + ((t.cnt - 1 - lane) & ~(kFrWave - 1));
    const u256 c = fr_load(a.layout, load_rec(src + i * 8));
    MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = c;
    NTT_NO_UNROLL while (i >= t.first + kFrWave) {
      i -= kFrWave;
      const u256 x = fr_load(a.layout, load_rec(src + i * 8));
      MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = Fr::add(Fr::mul(acc[j], a.step[p0 + j][6]), x);
    }
  }
  NTT_NO_UNROLL for (uint32_t s = 0; s < 6; ++s) {
    MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = Fr::add(acc[j], Fr::mul(a.step[p0 + j][s], wave_xor(acc[j], 1u << s)));
  }
  if (lane == 0) {
    MSM_UNROLL for (int j = 0; j < K; ++j) store_rec(a.totals + ((p0 + j) * a.tot_stride + blockIdx.x) * 8, acc[j]);
  }
}

template <int K>
__global__ void __launch_bounds__(kFrWave) fr_poly_points_scan_kernel(FrPolyPointsArgs a) {
  extern __shared__ uint32_t fr_lds[];
  const Image lds = image(fr_lds, a.tile_log);
  const uint32_t lane = threadIdx.x, p0 = blockIdx.y * K;
  const uint64_t v = blockIdx.x / a.tiles, b = blockIdx.x - v * a.tiles;
  const TilePlace t = tile_place(blockIdx.x, a.len, a.tiles, a.tile_log);
  const uint32_t per = 1u << lds.per_log, m0 = lane << lds.per_log;
  const uint32_t top = ((1u << a.tile_log) >> lds.per_log) - 1u;   // the lane of a full tile's last record
  const uint64_t at = ((uint64_t)blockIdx.y * a.src_stride + t.base + t.first) * 8;
  const bool weighted = K > 1 || a.level0;   // more than one point per block: level 0 only

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    lds_put(lds, m, fr_load(a.layout, load_rec(a.src + at + (uint64_t)m * 8)));
  __syncthreads();

  // s^(j) at the first record of the next tile: record b + 1 of this vector in point j's level above (read twice, at a
  // wave-uniform address, so that it does not hold K records of registers across the first walk)
  const bool has_carry = a.carry && b + 1 < a.tiles;
  auto carry = [&](int j) {
    return has_carry ? load_rec(a.carry + ((p0 + j) * a.tot_stride + blockIdx.x + 1) * 8) : u256_zero();
  };
  u256 acc[K];
  MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = fr_select(lane == top, carry(j), u256_zero());
  NTT_NO_UNROLL for (uint32_t i = per; i-- != 0;) {
    if (m0 + i >= t.cnt) continue;
    const u256 c = lds_get(lds, m0 + i);
    MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = Fr::add(Fr::mul(acc[j], a.z[p0 + j]), c);
  }
  // the suffix scans of the lane values: acc[j] becomes s^(j) at the lane's first record
  NTT_NO_UNROLL for (uint32_t s = 0; s < 6; ++s) {
    const uint32_t d = 1u << s;
    MSM_UNROLL for (int j = 0; j < K; ++j) {
      const u256 y = wave_down(acc[j], d);
      acc[j] = Fr::add(acc[j], Fr::mul(a.step[p0 + j][s], fr_select(lane + d < kFrWave, y, u256_zero())));
    }
  }
  if (a.totals && lane == 0) {
    MSM_UNROLL for (int j = 0; j < K; ++j) store_rec(a.totals + ((p0 + j) * a.tot_stride + blockIdx.x) * 8, acc[j]);
  }
  // s^(j) behind the lane's last record, then down the lane
  MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = fr_select(lane == top, carry(j), wave_down(acc[j], 1));
  NTT_NO_UNROLL for (uint32_t i = per; i-- != 0;) {
    const uint32_t m = m0 + i;
    if (m >= t.cnt) continue;
    const u256 c = lds_get(lds, m);
    // sum_j w_j s^(j)_(m+1) = sum_(j < K-1) w_j (s^(j) - s^(K-1)), for sum_j w_j = 0; one point: w = 1, no product
    u256 q = acc[0];
    if (K > 1) {
      q = Fr::mul(a.w[p0], Fr::sub(acc[0], acc[K - 1]));
      MSM_UNROLL for (int j = 1; j < K - 1; ++j) q = Fr::add(q, Fr::mul(a.w[p0 + j], Fr::sub(acc[j], acc[K - 1])));
    }
    MSM_UNROLL for (int j = 0; j < K; ++j) acc[j] = Fr::add(Fr::mul(acc[j], a.z[p0 + j]), c);
    lds_put(lds, m, weighted ? q : acc[0]);
  }
  __syncthreads();

  NTT_NO_UNROLL for (uint32_t m = lane; m < t.cnt; m += kFrWave)
    store_rec(a.dst + at + (uint64_t)m * 8, fr_store(a.layout, lds_get(lds, m)));
}

__global__ void __launch_bounds__(kFrMapThreads) fr_lincomb_kernel(int layout, u256 k, const uint32_t* A, uint64_t n,
                                                                    uint64_t n_vec, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (i >= n) return;
  u256 acc = fr_load(layout, load_rec(A + ((n_vec - 1) * n + i) * 8));
  NTT_NO_UNROLL for (uint64_t v = n_vec - 1; v-- != 0;) acc = Fr::add(Fr::mul(acc, k), fr_load(layout, load_rec(A + (v * n + i) * 8)));
  store_rec(out + i * 8, fr_store(layout, acc));
}

struct FrMatArgs {
  const uint32_t* row_off;   // n_rows + 1
  const uint2* ent;          // (column, dictionary id)
  const uint32_t* dict;      // raw records
  const uint4* segs;         // FrMatSeg
  const uint4* splits;       // FrMatSplit
  const uint32_t* x;
  uint32_t* y;
  uint32_t* partial;         // raw records
  uint64_t n_rows;
  uint32_t long_rows;
  int layout;
};

// acc + value x[column] for entry k of the matrix.  SIGNS: the dictionary ids 0 and 1 are pinned to 1 and r - 1 (fr_mat.hip.h),
// and such an entry is added or subtracted without the product and without its dictionary record
template <bool SIGNS>
__device__ __forceinline__ u256 mat_add_term(const FrMatArgs& a, const u256& acc, uint32_t k) {
  const uint2 e = a.ent[k];
  const u256 x = fr_load(a.layout, load_rec(a.x + (uint64_t)e.x * 8));
  if (SIGNS && e.y < 2u) return e.y ? Fr::sub(acc, x) : Fr::add(acc, x);
  return Fr::add(acc, Fr::mul(load_rec(a.dict + (uint64_t)e.y * 8), x));
}
__device__ __forceinline__ u256 wave_sum(u256 acc) {
  NTT_NO_UNROLL for (uint32_t d = kFrWave / 2; d != 0; d >>= 1) acc = Fr::add(acc, wave_xor(acc, d));
  return acc;
}

template <bool SIGNS>
__global__ void __launch_bounds__(kFrMapThreads) fr_mat_lane_kernel(FrMatArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (i >= a.n_rows) return;
  const uint32_t lo = a.row_off[i], hi = a.row_off[i + 1];
  if (hi - lo > a.long_rows) return;
  u256 acc = u256_zero();
  NTT_NO_UNROLL for (uint32_t k = lo; k < hi; ++k) acc = mat_add_term<SIGNS>(a, acc, k);
  store_rec(a.y + i * 8, fr_store(a.layout, acc));
}

template <bool SIGNS>
__global__ void __launch_bounds__(kFrWave) fr_mat_wave_kernel(FrMatArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint4 s = a.segs[blockIdx.x];   // row, first, count, slot
  u256 acc = u256_zero();
  NTT_NO_UNROLL for (uint32_t m = lane; m < s.z; m += kFrWave) acc = mat_add_term<SIGNS>(a, acc, s.y + m);
  acc = wave_sum(acc);
  if (lane != 0) return;
  if (s.w == kFrMatDirect) store_rec(a.y + (uint64_t)s.x * 8, fr_store(a.layout, acc));
  else store_rec(a.partial + (uint64_t)s.w * 8, acc);
}

__global__ void __launch_bounds__(kFrWave) fr_mat_fold_kernel(FrMatArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint4 s = a.splits[blockIdx.x];   // row, slot, count
  u256 acc = u256_zero();
  NTT_NO_UNROLL for (uint32_t m = lane; m < s.z; m += kFrWave) acc = Fr::add(acc, load_rec(a.partial + ((uint64_t)s.y + m) * 8));
  acc = wave_sum(acc);
  if (lane == 0) store_rec(a.y + (uint64_t)s.x * 8, fr_store(a.layout, acc));
}

// ---- multilinear tables and sumcheck rounds (fr_mle.hip.h) -------------------------------------------------------------------
struct FrMleRoundArgs {
  const uint32_t* in;
  uint32_t* partial;         // plane t: waves raw records
  uint64_t stride, h, waves;
  uint32_t chunk_log;
  int layout, order;
};
struct FrMleFoldArgs {
  const uint32_t* src;       // plane t: count raw records
  uint32_t* dst;             // plane t: groups raw records
  uint64_t count, groups;
};
struct FrMleEvalArgs {
  const uint32_t* src;
  uint32_t* dst;             // one raw record per tile
  uint64_t stride, tiles;    // records between the tables of src, tiles per table
  uint32_t tile_log, cnt_log;   // records per tile: 2^cnt_log <= 2^tile_log
  int layout;
  u256 r[kFrTileLog];        // the challenge of variable j of the tile
};
struct FrMleBindArgs {
  const uint32_t* in;
  uint32_t* out;
  uint64_t total;                  // outputs over all tables
  uint64_t in_stride, out_stride;  // records between tables
  uint64_t lane_step, rec_step;    // records between the first records of two outputs, and between the records of one
  uint32_t q_log;                  // outputs per table, as a power of two
  int in_layout, out_layout;
  u256 r[kFrMleBindVars];          // the challenge of bit b of the record's number within its output
};
struct FrMleEqArgs {
  uint32_t* out;
  uint32_t m;
  int layout;
  u256 f[kFrMleMaxVars][2];        // bit b of the index clear / set
};

// The fold of the 2^K records src, src + step, ...: bit b of a record's number meets r[b].  A tree in registers.
template <int K>
__device__ __forceinline__ u256 mle_tree(const uint32_t* src, uint64_t step, int layout, const u256* r) {
  if constexpr (K == 0) {
    return fr_load(layout, load_rec(src));
  } else {
    const u256 lo = mle_tree<K - 1>(src, step, layout, r);
    const u256 hi = mle_tree<K - 1>(src + (step << (K - 1)) * 8, step, layout, r);
    return fr_mle_fold(lo, hi, r[K - 1]);
  }
}

// two waves per SIMD: 256 registers, so that the four-table product stays clear of AGPRs and of scratch
template <int FORM, int K>
__global__ void __launch_bounds__(kFrWave, 2) fr_sumcheck_round_kernel(FrMleRoundArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x << a.chunk_log;
  const uint32_t cnt = 1u << a.chunk_log;
  FrMleSums<FORM, K> s;
  s.clear();
  NTT_NO_UNROLL for (uint32_t m = lane; m < cnt; m += kFrWave) {
    const uint64_t x = first + m;
    const uint64_t i_lo = a.order == kFrMleHigh ? x : 2 * x, i_hi = a.order == kFrMleHigh ? x + a.h : 2 * x + 1;
    u256 lo[K], hi[K];
    MSM_UNROLL for (int j = 0; j < K; ++j) {
      lo[j] = fr_load(a.layout, load_rec(a.in + ((uint64_t)j * a.stride + i_lo) * 8));
      hi[j] = fr_load(a.layout, load_rec(a.in + ((uint64_t)j * a.stride + i_hi) * 8));
    }
    s.add_pair(lo, hi);
  }
  MSM_UNROLL for (int t = 0; t < FrMleSums<FORM, K>::kValues; ++t) {
    const u256 sum = wave_sum(s.g[t]);
    if (lane == 0) store_rec(a.partial + ((uint64_t)t * a.waves + blockIdx.x) * 8, sum);
  }
}

// A round over a term list (fr_mle.hip.h, FrTermSums<D + 1>): the geometry and the partial planes of the kernel above
struct FrTermRoundArgs {
  const uint32_t* in;
  uint32_t* partial;         // plane t: waves raw records
  uint64_t stride, h, waves;
  uint32_t chunk_log;
  int layout, order;
  FrSumTerms terms;
};

template <int D>
__global__ void __launch_bounds__(kFrWave, 2) fr_sumcheck_terms_kernel(FrTermRoundArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x << a.chunk_log;
  const uint32_t cnt = 1u << a.chunk_log;
  FrTermSums<D + 1> s;
  s.clear();
  NTT_NO_UNROLL for (uint32_t m = lane; m < cnt; m += kFrWave) {
    const uint64_t x = first + m;
    const uint64_t i_lo = a.order == kFrMleHigh ? x : 2 * x, i_hi = a.order == kFrMleHigh ? x + a.h : 2 * x + 1;
    s.add_pair(a.terms, [&](uint32_t v, u256& lo, u256& hi) {
      lo = fr_load(a.layout, load_rec(a.in + ((uint64_t)v * a.stride + i_lo) * 8));
      hi = fr_load(a.layout, load_rec(a.in + ((uint64_t)v * a.stride + i_hi) * 8));
    });
  }
  MSM_UNROLL for (int t = 0; t <= D; ++t) {
    const u256 sum = wave_sum(s.g[t]);
    if (lane == 0) store_rec(a.partial + ((uint64_t)t * a.waves + blockIdx.x) * 8, sum);
  }
}

// A gate polynomial over rotated columns (fr_gate.hip.h): the image, k_acc and the geometry by value
struct FrGateArgs {
  const uint32_t* in;
  const uint32_t* acc;     // ACCUMULATE: the old records of out (out itself, or the staged copy of a host call)
  const uint32_t* scale;   // raw records, or null
  uint32_t* out;
  uint64_t n, stride;
  uint32_t period_mask;
  int layout, accumulate;
  u256 k_acc;
  FrGateTerms terms;
};

__global__ void __launch_bounds__(kFrMapThreads) fr_gate_kernel(FrGateArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (i >= a.n) return;
  u256 v = fr_gate_row(a.terms, i, a.n, [&](uint32_t col, uint64_t row) {
    return fr_load(a.layout, load_rec(a.in + ((uint64_t)col * a.stride + row) * 8));
  });
  if (a.accumulate) v = Fr::add(Fr::mul(a.k_acc, fr_load(a.layout, load_rec(a.acc + i * 8))), v);
  if (a.scale) v = Fr::mul(v, load_rec(a.scale + (i & a.period_mask) * 8));
  store_rec(a.out + i * 8, fr_store(a.layout, v));
}

__global__ void __launch_bounds__(kFrWave) fr_mle_fold_kernel(FrMleFoldArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t t = blockIdx.x / a.groups, g = blockIdx.x - t * a.groups;
  const uint64_t first = g << kFrMleFoldLog, left = a.count - first;
  const uint32_t cnt = left < (1u << kFrMleFoldLog) ? (uint32_t)left : (1u << kFrMleFoldLog);
  u256 acc = u256_zero();
  NTT_NO_UNROLL for (uint32_t m = lane; m < cnt; m += kFrWave) acc = Fr::add(acc, load_rec(a.src + (t * a.count + first + m) * 8));
  acc = wave_sum(acc);
  if (lane == 0) store_rec(a.dst + (uint64_t)blockIdx.x * 8, acc);
}

template <int PER_LOG>
__global__ void __launch_bounds__(kFrWave) fr_mle_eval_kernel(FrMleEvalArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t v = blockIdx.x / a.tiles, b = blockIdx.x - v * a.tiles;
  const uint32_t* src = a.src + (v * a.stride + (b << a.tile_log)) * 8;
  u256 acc = u256_zero();
  if ((lane >> a.cnt_log) == 0) acc = mle_tree<PER_LOG>(src + lane * 8, kFrWave, a.layout, a.r + 6);
  const uint32_t steps = a.cnt_log < 6u ? a.cnt_log : 6u;
  NTT_NO_UNROLL for (uint32_t s = 0; s < steps; ++s) {
    const u256 other = wave_xor(acc, 1u << s);
    const bool up = (lane >> s) & 1u;
    acc = fr_mle_fold(fr_select(up, other, acc), fr_select(up, acc, other), a.r[s]);
  }
  if (lane == 0) store_rec(a.dst + (uint64_t)blockIdx.x * 8, acc);
}

template <int K>
__global__ void __launch_bounds__(kFrMapThreads) fr_mle_bind_kernel(FrMleBindArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (idx >= a.total) return;
  const uint64_t v = idx >> a.q_log, i = idx - (v << a.q_log);
  const u256 x = mle_tree<K>(a.in + (v * a.in_stride + i * a.lane_step) * 8, a.rec_step, a.in_layout, a.r);
  store_rec(a.out + (v * a.out_stride + i) * 8, fr_store(a.out_layout, x));
}

// acc holds the factors of the bits below `bit`; the S bits from there double it
template <int S>
__device__ __forceinline__ void eq_spread(const FrMleEqArgs& a, const u256& acc, uint64_t i, uint32_t bit) {
  if constexpr (S == 0) {
    store_rec(a.out + i * 8, fr_store(a.layout, acc));
  } else {
    eq_spread<S - 1>(a, Fr::mul(acc, a.f[bit][0]), i, bit + 1);
    eq_spread<S - 1>(a, Fr::mul(acc, a.f[bit][1]), i + ((uint64_t)1 << bit), bit + 1);
  }
}

template <int S>
__global__ void __launch_bounds__(kFrMapThreads) fr_eq_table_kernel(FrMleEqArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  const uint32_t low = a.m - S;   // >= 1
  if (idx >> low) return;
  u256 acc = fr_select(idx & 1u, a.f[0][1], a.f[0][0]);
  NTT_NO_UNROLL for (uint32_t b = 1; b < low; ++b) acc = Fr::mul(acc, fr_select((idx >> b) & 1u, a.f[b][1], a.f[b][0]));
  eq_spread<S>(a, acc, idx, low);
}

// ---- Poseidon (fr_poseidon.hip.h) --------------------------------------------------------------------------------------------
struct FrPoseidonArgs {
  const uint32_t* image;     // the constants image: raw records
  const uint32_t* in;
  uint32_t* out;
  uint64_t n;                // lanes with work (the tail: nodes of its first level)
  uint32_t records;          // of the image
  uint32_t r_f, r_p;
  uint32_t levels;           // the tail: levels of the workgroup
  int layout;
  u256 tag;
};
struct FrMerklePathArgs {
  const uint32_t* leaves;
  const uint32_t* tree;
  const uint64_t* idx;
  uint32_t* out;
  uint64_t total, n_leaves;  // total = n_idx depth (arity - 1) records
  uint32_t depth, arity;
  int layout;
};

// The constants of a workgroup in LDS: every lane of a wave reads the same record, one broadcast of two b128 reads
struct PoseidonLds {
  const uint4* lds;
  __device__ __forceinline__ u256 record(uint32_t i) const {
    const uint4 a = lds[2 * i], b = lds[2 * i + 1];
    u256 x;
    x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w, x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
    return x;
  }
};
__device__ __forceinline__ PoseidonLds poseidon_stage(const FrPoseidonArgs& a, uint4* dst) {
  const uint4* src = (const uint4*)a.image;
  for (uint32_t i = threadIdx.x; i < 2 * a.records; i += kFrMapThreads) dst[i] = src[i];
  __syncthreads();
  return PoseidonLds{dst};
}

// One lane, one permutation: between the load of its inputs and the store of its outputs a lane reads LDS only.
template <int T, int KIND>
__device__ __forceinline__ void poseidon_lane(const FrPoseidonArgs& a, const PoseidonLds& c, const uint32_t* in, uint32_t* out,
                                              uint64_t i) {
  constexpr int IN = KIND == kPoseidonHash ? T - 1 : T, FIRST = T - IN;
  u256 s[T];
  if (KIND == kPoseidonHash) s[0] = a.tag;
  MSM_UNROLL for (int j = 0; j < IN; ++j) s[FIRST + j] = fr_load(a.layout, load_rec(in + (i * IN + j) * 8));
  poseidon_permute<T>(s, c, a.r_f, a.r_p);
  if (KIND == kPoseidonHash) {
    store_rec(out + i * 8, fr_store(a.layout, s[0]));
  } else {
    MSM_UNROLL for (int j = 0; j < T; ++j) store_rec(out + (i * T + j) * 8, fr_store(a.layout, s[j]));
  }
}

// One lane per permutation.  In place: a permutation's lane reads and writes its own t records.  A hash with t = 2 reads
// and writes record i alone.  For t >= 3 digest i lands on a record that lane i / (t - 1) reads, and no order holds between
// the lanes of two workgroups: the checks refuse every overlap of such a call (poseidon_call_check).
template <int T, int KIND>
__global__ void __launch_bounds__(kFrMapThreads) fr_poseidon_kernel(FrPoseidonArgs a) {
  extern __shared__ uint4 poseidon_lds[];
  const PoseidonLds c = poseidon_stage(a, poseidon_lds);
  const uint64_t i = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (i < a.n) poseidon_lane<T, KIND>(a, c, a.in, a.out, i);
}

// The last levels of a tree in one workgroup: level after level, a barrier between them; a level's nodes go to the tree
// and the level above reads them from there.  Every lane reaches every barrier: the trip counts are uniform.
template <int T>
__global__ void __launch_bounds__(kFrMapThreads) fr_poseidon_tail_kernel(FrPoseidonArgs a) {
  extern __shared__ uint4 poseidon_lds[];
  const PoseidonLds c = poseidon_stage(a, poseidon_lds);
  const uint32_t* src = a.in;
  uint32_t* dst = a.out;
  uint32_t count = (uint32_t)a.n;
  NTT_NO_UNROLL for (uint32_t level = 0; level < a.levels; ++level) {
    NTT_NO_UNROLL for (uint32_t i = threadIdx.x; i < count; i += kFrMapThreads) poseidon_lane<T, kPoseidonHash>(a, c, src, dst, i);
    __syncthreads();
    src = dst, dst += (uint64_t)count * 8, count /= (uint32_t)(T - 1);
  }
}

// One lane per sibling record: the walk up to its level, then one record of the leaves or of the tree
__global__ void __launch_bounds__(kFrMapThreads) fr_merkle_paths_kernel(FrMerklePathArgs a) {
  const uint64_t id = (uint64_t)blockIdx.x * kFrMapThreads + threadIdx.x;
  if (id >= a.total) return;
  const uint32_t sibs = a.arity - 1, per = a.depth * sibs;
  const uint64_t q = id / per;
  const uint32_t rem = (uint32_t)(id - q * per), level = rem / sibs, sib = rem - level * sibs;
  uint64_t pos = a.idx[q], count = a.n_leaves;
  const uint32_t* src = a.leaves;
  const uint32_t* above = a.tree;
  NTT_NO_UNROLL for (uint32_t k = 0; k < level; ++k) {
    pos /= a.arity, count /= a.arity;
    src = above, above += count * 8;
  }
  const uint32_t own = (uint32_t)(pos % a.arity);
  const uint64_t child = pos - own + (sib < own ? sib : sib + 1);
  store_rec(a.out + id * 8, fr_store(a.layout, fr_load(a.layout, load_rec(src + child * 8))));
}

template <int OP>
void launch_map_op(hipStream_t st, int layout, const u256& k, const void* a, const void* b, const void* c, size_t n, void* out) {
  hipLaunchKernelGGL(fr_map_kernel<OP>, dim3((uint32_t)((n + kFrMapThreads - 1) / kFrMapThreads)), dim3(kFrMapThreads), 0, st,
                     layout, k, (const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)c, (uint64_t)n, (uint32_t*)out);
}

void launch_reduce(hipStream_t st, const FrTileArgs& a, uint64_t n_vec, bool sum) {
  const dim3 grid((uint32_t)(a.tiles * n_vec));
  if (sum) hipLaunchKernelGGL(fr_tile_reduce_kernel<true>, grid, dim3(kFrWave), 0, st, a);
  else hipLaunchKernelGGL(fr_tile_reduce_kernel<false>, grid, dim3(kFrWave), 0, st, a);
}
void launch_scan(hipStream_t st, const FrTileArgs& a, uint64_t n_vec, bool sum) {
  const dim3 grid((uint32_t)(a.tiles * n_vec));
  if (sum) hipLaunchKernelGGL(fr_tile_scan_kernel<true>, grid, dim3(kFrWave), fr_image_bytes(a.tile_log), st, a);
  else hipLaunchKernelGGL(fr_tile_scan_kernel<false>, grid, dim3(kFrWave), fr_image_bytes(a.tile_log), st, a);
}

}  // namespace

void launch_fr_map(hipStream_t st, int op, int layout, const u256& k, const void* a, const void* b, const void* c, size_t n,
                   void* out) {
  switch (op) {
    case kFrAdd: return launch_map_op<kFrAdd>(st, layout, k, a, b, c, n, out);
    case kFrSub: return launch_map_op<kFrSub>(st, layout, k, a, b, c, n, out);
    case kFrMul: return launch_map_op<kFrMul>(st, layout, k, a, b, c, n, out);
    case kFrScale: return launch_map_op<kFrScale>(st, layout, k, a, b, c, n, out);
    case kFrAxpy: return launch_map_op<kFrAxpy>(st, layout, k, a, b, c, n, out);
    default: return launch_map_op<kFrMulsubScale>(st, layout, k, a, b, c, n, out);
  }
}

void launch_fr_shift(hipStream_t st, int layout, const u256& k, const void* a, size_t n, void* out) {
  launch_map_op<kFrShift>(st, layout, k, a, nullptr, nullptr, n, out);
}

uint32_t launch_fr_scan(hipStream_t st, const FrScanLaunch& c) {
  const FrScanPlan plan = fr_scan_plan(c.n, c.n_vec, c.tile_log);
  uint32_t* work = (uint32_t*)c.work;
  auto level = [&](uint32_t k) {   // the reads of level k, for a reduction or for the scan in place
    FrTileArgs a{};
    a.len = plan.len[k], a.tiles = plan.tiles[k], a.tile_log = c.tile_log;
    a.src = k == 0 ? (const uint32_t*)c.in : work + plan.offset[k] * 8;
    a.dst = k == 0 ? (uint32_t*)c.out : work + plan.offset[k] * 8;
    a.layout = k == 0 ? c.layout : kFrRaw;
    a.reverse = k == 0 && c.reverse;
    a.mode = k == 0 ? c.mode : kFrExclusive;
    if (k + 1 < plan.levels) a.carry = a.totals = work + plan.offset[k + 1] * 8;
    return a;
  };
  for (uint32_t k = 0; k + 1 < plan.levels; ++k) launch_reduce(st, level(k), c.n_vec, c.sum);
  for (uint32_t k = plan.levels; k-- != 0;) launch_scan(st, level(k), c.n_vec, c.sum);
  return plan.launches;
}

uint32_t launch_fr_poly(hipStream_t st, const FrPolyLaunch& c) {
  const FrScanPlan plan = fr_scan_plan(c.n, c.n_vec, c.tile_log);
  const uint32_t per_log = c.tile_log > 6u ? c.tile_log - 6u : 0u;
  uint32_t* work = (uint32_t*)c.work;
  // z^(2^j): level k works at the point z^(2^(T k))
  u256 pw[kFrPolyPowers];
  pw[0] = c.z;
  for (uint32_t j = 1; j < kFrPolyPowers; ++j) pw[j] = Fr::mul(pw[j - 1], pw[j - 1]);
  auto level = [&](uint32_t k, bool scan) {
    FrPolyArgs a{};
    a.len = plan.len[k], a.tiles = plan.tiles[k], a.tile_log = c.tile_log;
    a.src = k == 0 ? (const uint32_t*)c.in : work + plan.offset[k] * 8;
    a.layout = k == 0 ? c.layout : kFrRaw;
    const bool last = k + 1 == plan.levels;
    uint32_t* above = last ? work + plan.records * 8 : work + plan.offset[k + 1] * 8;
    const uint32_t e = c.tile_log * k;
    a.z = pw[e];
    if (scan) {
      a.dst = k == 0 ? (uint32_t*)c.out : work + plan.offset[k] * 8;
      a.shift = k == 0;
      a.carry = last ? nullptr : above;
      a.totals = last ? above : nullptr;
      for (uint32_t s = 0; s < 6; ++s) a.step[s] = pw[e + per_log + s];
    } else {
      a.totals = above;
      for (uint32_t s = 0; s < 7; ++s) a.step[s] = pw[e + s];
    }
    return a;
  };
  auto reduce = [&](uint32_t k) {
    const FrPolyArgs a = level(k, false);
    hipLaunchKernelGGL(fr_poly_reduce_kernel, dim3((uint32_t)(a.tiles * c.n_vec)), dim3(kFrWave), 0, st, a);
  };
  if (!c.divide) {
    for (uint32_t k = 0; k < plan.levels; ++k) reduce(k);
    return plan.levels;
  }
  for (uint32_t k = 0; k + 1 < plan.levels; ++k) reduce(k);
  for (uint32_t k = plan.levels; k-- != 0;) {
    const FrPolyArgs a = level(k, true);
    hipLaunchKernelGGL(fr_poly_scan_kernel, dim3((uint32_t)(a.tiles * c.n_vec)), dim3(kFrWave), fr_image_bytes(a.tile_log), st, a);
  }
  return plan.launches;
}

namespace {

// grid: x the tiles over all vectors, y the groups of K points
template <int K>
void launch_points_reduce(hipStream_t st, const FrPolyPointsArgs& a, uint64_t n_vec, uint32_t groups) {
  hipLaunchKernelGGL(fr_poly_points_reduce_kernel<K>, dim3((uint32_t)(a.tiles * n_vec), groups), dim3(kFrWave), 0, st, a);
}
template <int K>
void launch_points_scan(hipStream_t st, const FrPolyPointsArgs& a, uint64_t n_vec, uint32_t groups) {
  hipLaunchKernelGGL(fr_poly_points_scan_kernel<K>, dim3((uint32_t)(a.tiles * n_vec), groups), dim3(kFrWave),
                     fr_image_bytes(a.tile_log), st, a);
}
// level 0: all k points in one block; above: one block row per point
void launch_points(hipStream_t st, const FrPolyPointsArgs& a, uint64_t n_vec, uint32_t k, bool level0, bool scan) {
  if (!level0) return scan ? launch_points_scan<1>(st, a, n_vec, k) : launch_points_reduce<1>(st, a, n_vec, k);
  switch (k) {
    case 1: return scan ? launch_points_scan<1>(st, a, n_vec, 1) : launch_points_reduce<1>(st, a, n_vec, 1);
    case 2: return scan ? launch_points_scan<2>(st, a, n_vec, 1) : launch_points_reduce<2>(st, a, n_vec, 1);
    case 3: return scan ? launch_points_scan<3>(st, a, n_vec, 1) : launch_points_reduce<3>(st, a, n_vec, 1);
    case 4: return scan ? launch_points_scan<4>(st, a, n_vec, 1) : launch_points_reduce<4>(st, a, n_vec, 1);
    case 5: return scan ? launch_points_scan<5>(st, a, n_vec, 1) : launch_points_reduce<5>(st, a, n_vec, 1);
    case 6: return scan ? launch_points_scan<6>(st, a, n_vec, 1) : launch_points_reduce<6>(st, a, n_vec, 1);
    case 7: return scan ? launch_points_scan<7>(st, a, n_vec, 1) : launch_points_reduce<7>(st, a, n_vec, 1);
    default: return scan ? launch_points_scan<8>(st, a, n_vec, 1) : launch_points_reduce<8>(st, a, n_vec, 1);
  }
}

}  // namespace

uint32_t launch_fr_poly_points(hipStream_t st, const FrPolyPointsLaunch& c) {
  const FrScanPlan plan = fr_scan_plan(c.n, c.n_vec, c.tile_log);
  const uint32_t per_log = c.tile_log > 6u ? c.tile_log - 6u : 0u;
  uint32_t* work = (uint32_t*)c.work;
  uint32_t* values = work + fr_poly_points_values(plan, c.k) / 4;
  // z_j^(2^e): level l works at the points z_j^(2^(T l))
  u256 pw[kFrPolyMaxPoints][kFrPolyPowers], w[kFrPolyMaxPoints];
  for (uint32_t p = 0; p < c.k; ++p) {
    pw[p][0] = c.z[p];
    for (uint32_t e = 1; e < kFrPolyPowers; ++e) pw[p][e] = Fr::mul(pw[p][e - 1], pw[p][e - 1]);
  }
  if (c.divide) fr_poly_points_weights(c.z, c.k, w);
  auto level = [&](uint32_t l, bool scan) {
    FrPolyPointsArgs a{};
    a.len = plan.len[l], a.tiles = plan.tiles[l], a.tile_log = c.tile_log;
    a.src = l == 0 ? (const uint32_t*)c.in : work + plan.offset[l] * 8;
    a.src_stride = l == 0 ? 0 : plan.records;
    a.layout = l == 0 ? c.layout : kFrRaw;
    const bool last = l + 1 == plan.levels;
    uint32_t* above = last ? values : work + plan.offset[l + 1] * 8;
    a.tot_stride = last ? c.n_vec : plan.records;
    const uint32_t e = c.tile_log * l;
    for (uint32_t p = 0; p < c.k; ++p) {
      a.z[p] = pw[p][e];
      if (scan) {
        for (uint32_t s = 0; s < 6; ++s) a.step[p][s] = pw[p][e + per_log + s];
        if (l == 0) a.w[p] = w[p];
      } else {
        for (uint32_t s = 0; s < 7; ++s) a.step[p][s] = pw[p][e + s];
      }
    }
    if (scan) {
      a.dst = l == 0 ? (uint32_t*)c.out : work + plan.offset[l] * 8;
      a.level0 = l == 0;
      a.carry = last ? nullptr : above;
      a.totals = last ? above : nullptr;
    } else {
      a.totals = above;
    }
    return a;
  };
  const uint32_t reductions = c.divide ? plan.levels - 1 : plan.levels;
  for (uint32_t l = 0; l < reductions; ++l) launch_points(st, level(l, false), c.n_vec, c.k, l == 0, false);
  if (!c.divide) return plan.levels;
  for (uint32_t l = plan.levels; l-- != 0;) launch_points(st, level(l, true), c.n_vec, c.k, l == 0, true);
  return plan.launches;
}

void launch_fr_lincomb(hipStream_t st, int layout, const u256& k, const void* a, uint64_t n, uint64_t n_vec, void* out) {
  hipLaunchKernelGGL(fr_lincomb_kernel, dim3((uint32_t)((n + kFrMapThreads - 1) / kFrMapThreads)), dim3(kFrMapThreads), 0, st,
                     layout, k, (const uint32_t*)a, n, n_vec, (uint32_t*)out);
}

uint32_t launch_fr_matvec(hipStream_t st, const FrMatLaunch& c) {
  const uint8_t* img = (const uint8_t*)c.image;
  FrMatArgs a{};
  a.row_off = (const uint32_t*)(img + c.at.row_off), a.ent = (const uint2*)(img + c.at.ent);
  a.dict = (const uint32_t*)(img + c.at.dict), a.segs = (const uint4*)(img + c.at.segs);
  a.splits = (const uint4*)(img + c.at.splits);
  a.x = (const uint32_t*)c.x, a.y = (uint32_t*)c.y, a.partial = (uint32_t*)c.work;
  a.n_rows = c.n_rows, a.long_rows = c.long_rows, a.layout = c.layout;
  const dim3 lane_grid((uint32_t)((c.n_rows + kFrMapThreads - 1) / kFrMapThreads)), wave_grid((uint32_t)c.plan.segments);
  if (c.signs) hipLaunchKernelGGL(fr_mat_lane_kernel<true>, lane_grid, dim3(kFrMapThreads), 0, st, a);
  else hipLaunchKernelGGL(fr_mat_lane_kernel<false>, lane_grid, dim3(kFrMapThreads), 0, st, a);
  if (c.plan.segments && c.signs) hipLaunchKernelGGL(fr_mat_wave_kernel<true>, wave_grid, dim3(kFrWave), 0, st, a);
  else if (c.plan.segments) hipLaunchKernelGGL(fr_mat_wave_kernel<false>, wave_grid, dim3(kFrWave), 0, st, a);
  if (c.plan.split_rows) hipLaunchKernelGGL(fr_mat_fold_kernel, dim3((uint32_t)c.plan.split_rows), dim3(kFrWave), 0, st, a);
  return (uint32_t)c.plan.launches;
}

template <int FORM, int K>
void launch_round_form(hipStream_t st, const FrMleRoundArgs& a) {
  hipLaunchKernelGGL((fr_sumcheck_round_kernel<FORM, K>), dim3((uint32_t)a.waves), dim3(kFrWave), 0, st, a);
}

uint32_t launch_fr_sumcheck_round(hipStream_t st, const FrMleRoundLaunch& c) {
  const FrMleRoundPlan plan = fr_mle_round_plan(c.n, fr_mle_degree(c.form, c.n_vec) + 1, c.chunk_log);
  uint32_t* work = (uint32_t*)c.work;
  FrMleRoundArgs a{};
  a.in = (const uint32_t*)c.in, a.partial = work + plan.offset[0] * 8;
  a.stride = c.stride, a.h = c.n / 2, a.waves = plan.count[0], a.chunk_log = plan.chunk_log;
  a.layout = c.layout, a.order = c.order;
  if (c.form == kFrSumEqAbC) launch_round_form<kFrSumEqAbC, 4>(st, a);
  else if (c.n_vec == 1) launch_round_form<kFrSumProduct, 1>(st, a);
  else if (c.n_vec == 2) launch_round_form<kFrSumProduct, 2>(st, a);
  else if (c.n_vec == 3) launch_round_form<kFrSumProduct, 3>(st, a);
  else launch_round_form<kFrSumProduct, 4>(st, a);
  for (uint32_t k = 1; k < plan.levels; ++k) {
    FrMleFoldArgs f{};
    f.src = work + plan.offset[k - 1] * 8, f.dst = work + plan.offset[k] * 8;
    f.count = plan.count[k - 1], f.groups = plan.count[k];
    hipLaunchKernelGGL(fr_mle_fold_kernel, dim3((uint32_t)(f.groups * plan.values)), dim3(kFrWave), 0, st, f);
  }
  return plan.launches;
}

template <int D>
void launch_terms_degree(hipStream_t st, const FrTermRoundArgs& a) {
  hipLaunchKernelGGL((fr_sumcheck_terms_kernel<D>), dim3((uint32_t)a.waves), dim3(kFrWave), 0, st, a);
}

uint32_t launch_fr_sumcheck_terms(hipStream_t st, const FrTermRoundLaunch& c) {
  const uint32_t d = fr_sum_degree(c.terms);
  const uint64_t n = c.step ? c.n / 2 : c.n;   // the tables the sums run over
  const FrMleRoundPlan plan = fr_mle_round_plan(n, d + 1, c.chunk_log);
  uint32_t* work = (uint32_t*)c.work;
  uint32_t launches = plan.launches;
  FrTermRoundArgs a{};
  a.in = (const uint32_t*)c.in, a.partial = work + plan.offset[0] * 8;
  a.stride = c.stride, a.h = n / 2, a.waves = plan.count[0], a.chunk_log = plan.chunk_log;
  a.layout = c.layout, a.order = c.order, a.terms = c.terms;
  if (c.step) {   // the bind launch in front, on the same stream: the round reads what it wrote
    FrMleBindLaunch b{};
    b.in = c.in, b.out = c.out, b.work = nullptr, b.n = c.n, b.n_vec = c.n_vec, b.stride = c.stride, b.n_bind = 1;
    b.layout = c.layout, b.order = c.order, b.r[0] = c.r;
    launches += launch_fr_mle_bind(st, b);
    a.in = (const uint32_t*)c.out;
  }
  switch (d) {
    case 1: launch_terms_degree<1>(st, a); break;
    case 2: launch_terms_degree<2>(st, a); break;
    case 3: launch_terms_degree<3>(st, a); break;
    case 4: launch_terms_degree<4>(st, a); break;
    case 5: launch_terms_degree<5>(st, a); break;
    case 6: launch_terms_degree<6>(st, a); break;
    default: launch_terms_degree<7>(st, a); break;
  }
  for (uint32_t k = 1; k < plan.levels; ++k) {
    FrMleFoldArgs f{};
    f.src = work + plan.offset[k - 1] * 8, f.dst = work + plan.offset[k] * 8;
    f.count = plan.count[k - 1], f.groups = plan.count[k];
    hipLaunchKernelGGL(fr_mle_fold_kernel, dim3((uint32_t)(f.groups * plan.values)), dim3(kFrWave), 0, st, f);
  }
  return launches;
}

void launch_fr_gate(hipStream_t st, const FrGateLaunch& c) {
  FrGateArgs a{};
  a.in = (const uint32_t*)c.in, a.acc = (const uint32_t*)c.acc, a.scale = (const uint32_t*)c.scale, a.out = (uint32_t*)c.out;
  a.n = c.n, a.stride = c.stride, a.period_mask = c.scale ? c.period - 1 : 0;
  a.layout = c.layout, a.accumulate = c.accumulate, a.k_acc = c.k_acc, a.terms = c.terms;
  hipLaunchKernelGGL(fr_gate_kernel, dim3((uint32_t)((c.n + kFrMapThreads - 1) / kFrMapThreads)), dim3(kFrMapThreads), 0, st, a);
}

uint32_t launch_fr_mle_eval(hipStream_t st, const FrMleEvalLaunch& c) {
  const FrScanPlan plan = fr_scan_plan(c.n, c.n_vec, c.tile_log);
  uint32_t* work = (uint32_t*)c.work;
  uint32_t var = 0;
  for (uint32_t k = 0; k < plan.levels; ++k) {
    const bool last = k + 1 == plan.levels;
    FrMleEvalArgs a{};
    a.src = k == 0 ? (const uint32_t*)c.in : work + plan.offset[k] * 8;
    a.dst = last ? work + plan.records * 8 : work + plan.offset[k + 1] * 8;
    a.stride = k == 0 ? c.stride : plan.len[k], a.tiles = plan.tiles[k];
    a.tile_log = c.tile_log;
    a.cnt_log = fr_mle_log2(plan.len[k] < ((uint64_t)1 << c.tile_log) ? plan.len[k] : (uint64_t)1 << c.tile_log);
    a.layout = k == 0 ? c.layout : kFrRaw;
    // lane l holds the records l, l + 64, ...: variables 0 .. 5 of the tile are the lane's bits, the rest its tree's
    for (uint32_t j = 0; j < a.cnt_log; ++j) a.r[j] = c.r[var + j];
    var += a.cnt_log;
    const dim3 grid((uint32_t)(a.tiles * c.n_vec));
    switch (fr_mle_per_log((uint64_t)1 << a.cnt_log)) {
      case 0: hipLaunchKernelGGL(fr_mle_eval_kernel<0>, grid, dim3(kFrWave), 0, st, a); break;
      case 1: hipLaunchKernelGGL(fr_mle_eval_kernel<1>, grid, dim3(kFrWave), 0, st, a); break;
      case 2: hipLaunchKernelGGL(fr_mle_eval_kernel<2>, grid, dim3(kFrWave), 0, st, a); break;
      default: hipLaunchKernelGGL(fr_mle_eval_kernel<3>, grid, dim3(kFrWave), 0, st, a); break;
    }
  }
  return plan.levels;
}

uint32_t launch_fr_mle_bind(hipStream_t st, const FrMleBindLaunch& c) {
  const FrMleBindPlan plan = fr_mle_bind_plan(c.order, c.n, c.n_vec, c.n_bind);
  const bool high = c.order == kFrMleHigh;
  uint64_t len = c.n;
  uint32_t used = 0;
  const uint32_t* src = (const uint32_t*)c.in;
  uint64_t src_stride = c.stride;
  for (uint32_t k = 0; k < plan.launches; ++k) {
    const uint32_t vars = plan.vars[k];
    const bool last = k + 1 == plan.launches;
    // HIGH: into the output, and in place from there.  LOW: output and workspace in turn, the last launch into the output.
    const bool to_out = high || ((plan.launches - 1 - k) & 1u) == 0;
    const uint64_t q = len >> vars;
    FrMleBindArgs a{};
    a.in = src, a.out = to_out ? (uint32_t*)c.out : (uint32_t*)c.work;
    a.total = q * c.n_vec, a.q_log = fr_mle_log2(q);
    a.in_stride = src_stride, a.out_stride = to_out ? c.stride : q;
    a.lane_step = high ? 1 : (uint64_t)1 << vars, a.rec_step = high ? q : 1;
    a.in_layout = k == 0 ? c.layout : kFrRaw, a.out_layout = last ? c.layout : kFrRaw;
    // step s of the launch binds bit s of the record's number (LOW) or bit vars - 1 - s (HIGH)
    for (uint32_t s = 0; s < vars; ++s) a.r[high ? vars - 1 - s : s] = c.r[used + s];
    const dim3 grid((uint32_t)((a.total + kFrMapThreads - 1) / kFrMapThreads));
    if (vars == 1) hipLaunchKernelGGL(fr_mle_bind_kernel<1>, grid, dim3(kFrMapThreads), 0, st, a);
    else if (vars == 2) hipLaunchKernelGGL(fr_mle_bind_kernel<2>, grid, dim3(kFrMapThreads), 0, st, a);
    else hipLaunchKernelGGL(fr_mle_bind_kernel<3>, grid, dim3(kFrMapThreads), 0, st, a);
    src = a.out, src_stride = a.out_stride, len = q, used += vars;
  }
  return plan.launches;
}

void launch_fr_eq_table(hipStream_t st, int layout, const u256* point_by_bit, uint32_t m, void* out) {
  FrMleEqArgs a{};
  a.out = (uint32_t*)out, a.m = m, a.layout = layout;
  for (uint32_t b = 0; b < m; ++b) a.f[b][0] = Fr::sub(Fr::one(), point_by_bit[b]), a.f[b][1] = point_by_bit[b];
  const bool wide = m >= kFrMleEqWideFrom;
  const uint64_t lanes = (uint64_t)1 << (wide ? m - kFrMleEqSpread : m);
  const dim3 grid((uint32_t)((lanes + kFrMapThreads - 1) / kFrMapThreads));
  if (wide) hipLaunchKernelGGL(fr_eq_table_kernel<(int)kFrMleEqSpread>, grid, dim3(kFrMapThreads), 0, st, a);
  else hipLaunchKernelGGL(fr_eq_table_kernel<0>, grid, dim3(kFrMapThreads), 0, st, a);
}

namespace {

FrPoseidonArgs poseidon_args(const PoseidonLaunch& c, const void* in, uint64_t n, void* out) {
  FrPoseidonArgs a{};
  a.image = (const uint32_t*)c.image, a.in = (const uint32_t*)in, a.out = (uint32_t*)out, a.n = n;
  a.records = poseidon_image_records(c.t, c.r_f + c.r_p), a.r_f = c.r_f, a.r_p = c.r_p;
  a.layout = c.layout, a.tag = c.tag;
  return a;
}

template <int KIND>
void launch_poseidon_kind(hipStream_t st, uint32_t t, const FrPoseidonArgs& a) {
  const dim3 grid((uint32_t)((a.n + kFrMapThreads - 1) / kFrMapThreads)), block(kFrMapThreads);
  const uint32_t lds = a.records * 32;
  if (t == 2) hipLaunchKernelGGL((fr_poseidon_kernel<2, KIND>), grid, block, lds, st, a);
  else if (t == 3) hipLaunchKernelGGL((fr_poseidon_kernel<3, KIND>), grid, block, lds, st, a);
  else if (t == 4) hipLaunchKernelGGL((fr_poseidon_kernel<4, KIND>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((fr_poseidon_kernel<5, KIND>), grid, block, lds, st, a);
}

}  // namespace

void launch_poseidon(hipStream_t st, const PoseidonLaunch& c, int kind, const void* in, uint64_t n, void* out) {
  const FrPoseidonArgs a = poseidon_args(c, in, n, out);
  if (kind == kPoseidonHash) launch_poseidon_kind<kPoseidonHash>(st, c.t, a);
  else launch_poseidon_kind<kPoseidonPermute>(st, c.t, a);
}

uint32_t launch_poseidon_tree(hipStream_t st, const PoseidonLaunch& c, const void* leaves, uint64_t n_leaves, uint32_t top_log,
                              void* tree) {
  const PoseidonTreePlan plan = poseidon_tree_plan(n_leaves, c.t - 1, top_log);
  const uint32_t* src = (const uint32_t*)leaves;
  uint32_t* dst = (uint32_t*)tree;
  const uint32_t level_launches = plan.launches - 1;
  for (uint32_t k = 0; k < level_launches; ++k) {
    launch_poseidon_kind<kPoseidonHash>(st, c.t, poseidon_args(c, src, plan.count[k], dst));
    src = dst, dst += plan.count[k] * 8;
  }
  FrPoseidonArgs a = poseidon_args(c, src, plan.count[level_launches], dst);
  a.levels = plan.tail_levels;
  const dim3 one(1), block(kFrMapThreads);
  const uint32_t lds = a.records * 32;
  if (c.t == 3) hipLaunchKernelGGL(fr_poseidon_tail_kernel<3>, one, block, lds, st, a);
  else if (c.t == 4) hipLaunchKernelGGL(fr_poseidon_tail_kernel<4>, one, block, lds, st, a);
  else hipLaunchKernelGGL(fr_poseidon_tail_kernel<5>, one, block, lds, st, a);
  return plan.launches;
}

void launch_merkle_paths(hipStream_t st, int layout, uint32_t arity, uint32_t depth, const void* leaves, uint64_t n_leaves,
                         const void* tree, const void* idx, uint64_t n_idx, void* out) {
  FrMerklePathArgs a{};
  a.leaves = (const uint32_t*)leaves, a.tree = (const uint32_t*)tree, a.idx = (const uint64_t*)idx, a.out = (uint32_t*)out;
  a.total = n_idx * depth * (arity - 1), a.n_leaves = n_leaves, a.depth = depth, a.arity = arity, a.layout = layout;
  hipLaunchKernelGGL(fr_merkle_paths_kernel, dim3((uint32_t)((a.total + kFrMapThreads - 1) / kFrMapThreads)), dim3(kFrMapThreads),
                     0, st, a);
}

uint32_t launch_fr_inv_products(hipStream_t st, int layout, const void* in, uint64_t n, uint32_t tile_log, void* work_v) {
  const FrInvPlan ip = fr_inv_plan(n, tile_log);
  uint32_t* work = (uint32_t*)work_v;
  uint32_t* count = work + (ip.p_off + ip.tiles) * 8;
  (void)hipMemsetAsync(count, 0, 32, st);
  FrTileArgs a{};
  a.src = (const uint32_t*)in, a.totals = work + ip.t_off * 8, a.zeros = (unsigned long long*)count;
  a.len = n, a.tiles = ip.tiles, a.tile_log = ip.tile_log, a.layout = layout, a.zero_one = 1;
  launch_reduce(st, a, 1, false);
  FrScanLaunch s{};
  s.in = work + ip.t_off * 8, s.work = work + ip.scan_off * 8;
  s.n = ip.tiles, s.n_vec = 1, s.tile_log = tile_log, s.layout = kFrRaw, s.mode = kFrInclusive;
  s.out = work + ip.p_off * 8;
  uint32_t launches = 1 + launch_fr_scan(st, s);
  s.out = work + ip.s_off * 8, s.reverse = true;
  return launches + launch_fr_scan(st, s);
}

void launch_fr_inv_apply(hipStream_t st, int layout, const void* in, uint64_t n, uint32_t tile_log, const void* work_v,
                         const u256& t_inv, void* out) {
  const FrInvPlan ip = fr_inv_plan(n, tile_log);
  const uint32_t* work = (const uint32_t*)work_v;
  FrInvArgs a{};
  a.src = (const uint32_t*)in, a.dst = (uint32_t*)out, a.P = work + ip.p_off * 8, a.S = work + ip.s_off * 8;
  a.len = n, a.tiles = ip.tiles, a.tile_log = ip.tile_log, a.layout = layout, a.t_inv = t_inv;
  hipLaunchKernelGGL(fr_inv_apply_kernel, dim3((uint32_t)ip.tiles), dim3(kFrWave), 2 * fr_image_bytes(a.tile_log), st, a);
}

}  // namespace msm_amd
