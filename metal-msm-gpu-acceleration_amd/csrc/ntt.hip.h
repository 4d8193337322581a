// Number-theoretic transform over BN254 Fr: the bodies shared by the kernels (k_ntt.hip), the host twin (host_ntt.hip)
// and the host driver (msm_host.hip).  Everything here compiles for the device and for the host (MSM_HD).
//
// n = 2^L.  The transform is a decimation-in-frequency (Gentleman-Sande) radix-2 network on natural-order input: level
// l (0 = first) pairs index i with i + h, h = n >> (l + 1), for every i whose bit (L - 1 - l) is clear:
//     a[i], a[i + h]  <-  a[i] + a[i + h],  (a[i] - a[i + h]) w^((i mod h) << l)          (ntt_bfly)
// After L levels position bitrev_L(k) holds X[k] = sum_i a[i] w^(i k).  The last pass of a plan stores to natural order:
// FORWARD writes X[k] to k, INVERSE writes n^-1 X[k] to (n - k) mod n, which is the sum with w^-1 -- one table of
// w^j, j < n/2, serves both directions.
//
// Plan (ntt_plan).  The L levels are cut into P = ceil(L / T) passes of L/P or L/P + 1 levels (the longer ones first), T
// = the tile size in bits (kNttTileLog = 10, MSM_AMD_NTT_TILE_LOG lowers it).  A pass of t levels starting at level l0
// works on tiles of 2^t elements at stride s = 2^sigma, sigma = L - l0 - t.  A workgroup always holds 2^T elements: 2^(T-t)
// tiles that are neighbours in memory (consecutive low index bits first, then consecutive blocks), over all vectors of
// the batch as one flat index space -- so short passes, short transforms and batches of short vectors all fill the
// workgroup, and the gathers of a strided pass read 2^(T-t) consecutive records.  ntt_slot_index maps the workgroup's
// slot m < 2^T to the global element; slots are ordered by global significance, so that consecutive lanes touch
// consecutive records whenever the pass allows it.
//
// Fused work.  The first pass reads the caller's records (ntt_load: five reduce_once, to_mont for CANON_LE) and, FORWARD
// with a shift, multiplies a[i] by g^i; the last pass applies n^-1 g^-i (INVERSE) and writes the caller's layout
// (ntt_store).  Powers of g: a table of g^(d 16^w), d < 16, w < 7 (kNttPowEntries records, built on the host per call);
// a thread takes the power of its first slot with at most 6 products (ntt_pow) and steps to its other slots with one
// product each.  INVERSE: the factor of output position j = (n - k) mod n is g^-j n^-1 = (n^-1 g^-n) g^k for k != 0.
#pragma once
#include "bn254_fq.hip.h"

#if defined(__HIPCC__)
#define NTT_NO_UNROLL _Pragma("unroll 1")
#else
#define NTT_NO_UNROLL
#endif

namespace msm_amd {

constexpr uint32_t kNttMaxLog = 28;        // r - 1 = 2^28 t, t odd
constexpr uint32_t kNttTileLog = 10;       // 2^10 elements per workgroup: 32 KiB of LDS
constexpr uint32_t kNttThreads = 256;
constexpr uint32_t kNttPowWindows = 7, kNttPowEntries = 16 * kNttPowWindows;   // 4-bit windows over a 28-bit exponent
constexpr int kNttRootArk = 0, kNttRootH2c = 1;
constexpr int kNttForward = 0, kNttInverse = 1;
constexpr int kNttMontLe = 0, kNttCanonLe = 1;

struct NttPlan {
  uint32_t passes;        // >= 1 (log_n = 0: one pass of no levels, the fused conversions only)
  uint32_t levels[28];    // per pass
};

// tile_log: 2 .. kNttTileLog
inline NttPlan ntt_plan(uint32_t log_n, uint32_t tile_log) {
  NttPlan p{};
  p.passes = log_n == 0 ? 1 : (log_n + tile_log - 1) / tile_log;
  for (uint32_t k = 0; k < p.passes; ++k) p.levels[k] = log_n / p.passes + (k < log_n % p.passes ? 1u : 0u);
  return p;
}

// What one pass needs to place its elements.
struct NttPass {
  uint32_t log_n;       // L
  uint32_t level0;      // first level of the pass
  uint32_t levels;      // t
  uint32_t tile_log;    // T
  uint32_t sigma;       // log2 of the tile stride: L - level0 - t
  uint32_t low;         // min(sigma, T - t): index bits below the tile bits that the workgroup holds
};

MSM_HD NttPass ntt_pass(uint32_t log_n, uint32_t level0, uint32_t levels, uint32_t tile_log) {
  NttPass p;
  p.log_n = log_n, p.level0 = level0, p.levels = levels, p.tile_log = tile_log;
  p.sigma = log_n - level0 - levels;
  p.low = p.sigma < tile_log - levels ? p.sigma : tile_log - levels;
  return p;
}

// Slot m < 2^T of workgroup wg -> flat element index v * n + i over the batch (64 bits: the caller compares it with
// n_vec * n).  Slot bits: [0, low) low index bits, [low, low + t) the tile position q, the rest further tiles.
MSM_HD uint64_t ntt_slot_index(const NttPass& p, uint64_t wg, uint32_t m) {
  const uint32_t t = p.levels;
  const uint32_t q = (m >> p.low) & ((1u << t) - 1u);
  const uint32_t tl = ((m >> (p.low + t)) << p.low) | (m & ((1u << p.low) - 1u));
  const uint64_t tile = (wg << (p.tile_log - t)) + tl;   // over the batch: n_vec * n / 2^t tiles
  const uint64_t lo = tile & (((uint64_t)1 << p.sigma) - 1u);
  return ((tile >> p.sigma) << (t + p.sigma)) | ((uint64_t)q << p.sigma) | lo;
}

MSM_HD uint32_t ntt_bitrev(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  NTT_NO_UNROLL for (uint32_t b = 0; b < bits; ++b) {
    r = (r << 1) | (x & 1u);
    x >>= 1;
  }
  return r;
}

// The butterfly of one level: tw = w^((i mod h) << l) in Montgomery form.
MSM_HD void ntt_bfly(u256& a, u256& b, const u256& tw) {
  const u256 s = Fr::add(a, b);
  b = Fr::mul(Fr::sub(a, b), tw);
  a = s;
}

// index of the twiddle of element i (bit L-1-l clear) at level l, into the table of w^j, j < n/2
MSM_HD uint32_t ntt_twiddle_index(uint32_t i, uint32_t log_n, uint32_t level) {
  const uint32_t h = (1u << (log_n - level - 1u));
  return (i & (h - 1u)) << level;
}

// One record of the caller -> fully reduced Montgomery residue.  Any 256-bit value is taken mod r (2^256 / r < 6).
MSM_HD u256 ntt_load(int layout, const uint32_t* rec) {
  u256 k;
  MSM_UNROLL for (int i = 0; i < 8; ++i) k.v[i] = rec[i];
  NTT_NO_UNROLL for (int i = 0; i < 5; ++i) k = Fr::reduce_once(k);
  return layout == kNttCanonLe ? Fr::to_mont(k) : k;
}

MSM_HD void ntt_store(int layout, const u256& x, uint32_t* rec) {
  const u256 k = layout == kNttCanonLe ? Fr::from_mont(x) : x;
  MSM_UNROLL for (int i = 0; i < 8; ++i) rec[i] = k.v[i];
}

// base^e from the window table tab[16 w + d] = base^(d 16^w), e < 2^28: one load and at most 6 products
MSM_HD u256 ntt_pow(const u256* tab, uint32_t e) {
  u256 acc = tab[e & 15u];
  e >>= 4;
  NTT_NO_UNROLL for (uint32_t w = 1; e != 0; ++w, e >>= 4) {
    if (e & 15u) acc = Fr::mul(acc, tab[16u * w + (e & 15u)]);
  }
  return acc;
}
// base^(2^b) from the same table
MSM_HD u256 ntt_pow2(const u256* tab, uint32_t b) { return tab[16u * (b >> 2) + (1u << (b & 3u))]; }

// The factors a call fuses into its first or last pass (host side of ntt_pow: everything Montgomery).
struct NttScale {
  u256 c0;   // INVERSE: n^-1 g^-n, the factor next to g^k for k != 0
  u256 c1;   // INVERSE: n^-1, the factor of k = 0
};

// ---- host-only arithmetic (roots, inverses, the power table) ---------------------------------------------------------
inline u256 ntt_fr_pow(const u256& base, const u256& e) {   // base Montgomery, e an integer
  u256 r = Fr::one();
  for (int i = 255; i >= 0; --i) {
    r = Fr::sqr(r);
    if ((e.v[i >> 5] >> (i & 31)) & 1u) r = Fr::mul(r, base);
  }
  return r;
}
inline u256 ntt_fr_small(uint32_t x) {
  u256 k = u256_zero();
  k.v[0] = x;
  return Fr::to_mont(k);
}
inline u256 ntt_fr_inv(const u256& a) {   // a != 0: a^(r - 2)
  u256 e = Fr::modulus();
  e.v[0] -= 2u;   // the low word of r is 0xF0000001
  return ntt_fr_pow(a, e);
}
// rho = g^t, g = 5 (ROOT_ARK) or 7 (ROOT_H2C), t = (r - 1) / 2^28; Montgomery
inline u256 ntt_rho(int root) {
  u256 e = Fr::modulus();
  e.v[0] -= 1u;
  return ntt_fr_pow(ntt_fr_small(root == kNttRootArk ? 5u : 7u), u256_shr(e, kNttMaxLog));
}
// w = rho^(2^(28 - log_n))
inline u256 ntt_omega(int root, uint32_t log_n) {
  u256 w = ntt_rho(root);
  for (uint32_t k = log_n; k < kNttMaxLog; ++k) w = Fr::sqr(w);
  return w;
}
inline void ntt_pow_table(const u256& base, u256* tab) {
  u256 b = base;
  for (uint32_t w = 0; w < kNttPowWindows; ++w) {
    tab[16 * w] = Fr::one();
    for (uint32_t d = 1; d < 16; ++d) tab[16 * w + d] = Fr::mul(tab[16 * w + d - 1], b);
    b = Fr::mul(tab[16 * w + 15], b);
  }
}
// The shift of a call: g (already reduced, Montgomery, non-zero) -> the power table and the factors.  FORWARD and
// INVERSE both use powers of g itself (see the head of this file).
inline void ntt_shift_setup(const u256& g, int direction, uint32_t log_n, u256* tab, NttScale* sc) {
  ntt_pow_table(g, tab);
  u256 n = u256_zero();
  n.v[log_n >> 5] = 1u << (log_n & 31);
  const u256 n_inv = ntt_fr_inv(Fr::to_mont(n));
  sc->c1 = direction == kNttInverse ? n_inv : Fr::one();
  u256 gn = g;
  for (uint32_t k = 0; k < log_n; ++k) gn = Fr::sqr(gn);
  sc->c0 = direction == kNttInverse ? Fr::mul(n_inv, ntt_fr_inv(gn)) : Fr::one();
}

}  // namespace msm_amd
