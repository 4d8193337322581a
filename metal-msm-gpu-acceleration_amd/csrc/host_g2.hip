// Host code of the G2 MSM (no GPU): the Horner pass of a device G2 MSM, the CPU G2 MSM msm_amd_host_msm_g2 (a plain
// windowed bucket method on the 64-bit host arithmetic of host_fq2_64.h, the CPU counterpart and a second
// implementation for the tests), the progression generator of the tests and the host twin of the raw G2 test ops.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/msm_amd.h"
#include "host_fq2_64.h"
#include "launch_g2.h"
#include "test_ops_g2.hip.h"
#include "compress_points.hip.h"
#include "scalar_width.hip.h"

namespace msm_amd {

namespace {

h64::Jac2 load_jac2(const Jacobian2& p) {
  h64::Jac2 r;
  std::memcpy(&r, &p, sizeof r);
  return r;
}

// A record of an external G2 layout -> host affine (identity = all zero)
bool read_g2_point(int layout, const uint8_t* points, size_t i, h64::Aff2& out) {
  switch (layout) {
    case MSM_AMD_G2_POINT_H2C_AFFINE:
      std::memcpy(&out, points + i * 128, 128);
      return true;
    case MSM_AMD_G2_POINT_ARK_AFFINE:
      std::memcpy(&out, points + i * 136, 128);
      if (points[i * 136 + 128] != 0) std::memset(&out, 0, sizeof out);
      return true;
  }
  return false;
}

// canonical scalar k < r of an external scalar record
u256 read_scalar(int layout, const uint8_t* scalars, size_t i) {
  u256 k;
  if (layout == MSM_AMD_SCALAR_CANON_BE32) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(scalars + i * 32);
    for (int j = 0; j < 8; ++j) k.v[j] = w[7 - j];
  } else {
    std::memcpy(&k, scalars + i * 32, 32);
  }
  if (layout == MSM_AMD_SCALAR_MONT_LE) return Fr::from_mont(k);
  for (int t = 0; t < 5; ++t) k = Fr::reduce_once(k);   // raw canonical integers may exceed r (2^256 / r < 6)
  return k;
}

unsigned pick_threads(int threads) {
  if (threads > 0) return (unsigned)threads;
  return std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
}

}  // namespace

// Window value  W_w = partial[w][lb] + sum_k 2^k partial[w][k]  and the Horner sum over windows, one pass over bit
// positions: host_combine (msm_host.hip) on G2.
Jacobian2 host_combine_g2(const Jacobian2* partial, const Plan& p) {
  const uint32_t top = p.c * (p.W - 1) + p.lb;
  h64::Jac2 acc = h64::identity2();
  for (int pos = (int)top; pos >= 0; --pos) {
    acc = h64::jdouble2(acc);
    for (uint32_t w = std::min((uint32_t)pos / p.c, p.W - 1);; --w) {
      const uint32_t k = (uint32_t)pos - p.c * w;
      if (k > p.lb) break;
      const Jacobian2* pw = partial + (size_t)w * (p.lb + 1);
      if (k == 0) acc = h64::jadd2(acc, load_jac2(pw[p.lb]));
      if (k < p.lb) acc = h64::jadd2(acc, load_jac2(pw[k]));
      if (w == 0) break;
    }
  }
  const h64::Jac2 nrm = h64::normalise2(acc);
  Jacobian2 r;
  std::memcpy(&r, &nrm, sizeof r);
  return r;
}

}  // namespace msm_amd

extern "C" {

size_t msm_amd_g2_point_bytes(int layout) {
  switch (layout) {
    case MSM_AMD_G2_POINT_H2C_AFFINE: return 128;
    case MSM_AMD_G2_POINT_ARK_AFFINE: return 136;
  }
  return 0;
}

// CPU G2 MSM: unsigned c-bit windows, one bucket set per window, Jacobian + affine bucket additions, running sums;
// windows are spread over `threads` host threads.
// width.bounded(): ceil(bits / c) windows; a signed call folds k > (r - 1) / 2 to r - k and negates the base instead.
static int host_msm_g2_entry(int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
                             int threads, msm_amd::WidthBound width, void* out192) {
  using namespace msm_amd;
  if (!out192 || msm_amd_g2_point_bytes(g2_point_layout) == 0) return MSM_AMD_INPUT_ERROR;
  if (scalar_layout != MSM_AMD_SCALAR_MONT_LE && scalar_layout != MSM_AMD_SCALAR_CANON_LE &&
      scalar_layout != MSM_AMD_SCALAR_CANON_BE32)
    return MSM_AMD_INPUT_ERROR;
  if (n > 0 && (!scalars || !points)) return MSM_AMD_INPUT_ERROR;
  const uint8_t* sc = (const uint8_t*)scalars;
  const uint8_t* pt = (const uint8_t*)points;
  std::vector<u256> k(n);
  std::vector<h64::Aff2> base(n);
  for (size_t i = 0; i < n; ++i) {
    read_g2_point(g2_point_layout, pt, i, base[i]);
    k[i] = read_scalar(scalar_layout, sc, i);
    if (width.bounded()) {
      uint32_t flip;
      k[i] = scalar_magnitude(k[i], width.sign, &flip);
      if (u256_bit_length(k[i]) > width.bits) return MSM_AMD_INPUT_ERROR;   // beyond the bound: the output stays as it was
      if (flip) base[i].y = h64::neg2(base[i].y);
    }
    if (h64::aff2_is_identity(base[i])) k[i] = u256_zero();
  }
  uint32_t c = 3;
  while (c < 16 && ((size_t)1 << (c + 3)) < n) ++c;
  const uint32_t W = (width.width() + c - 1) / c;
  std::vector<h64::Jac2> win(W);
  std::atomic<uint32_t> next{0};
  auto worker = [&]() {
    std::vector<h64::Jac2> bucket(((size_t)1 << c) - 1);
    for (;;) {
      const uint32_t w = next.fetch_add(1);
      if (w >= W) break;
      std::fill(bucket.begin(), bucket.end(), h64::identity2());
      for (size_t i = 0; i < n; ++i) {
        const uint32_t d = u256_extract_bits(k[i], w * c, std::min(c, 256 - w * c));
        if (d) bucket[d - 1] = h64::jmadd2(bucket[d - 1], base[i]);
      }
      h64::Jac2 run = h64::identity2(), sum = h64::identity2();
      for (size_t b = bucket.size(); b-- > 0;) {
        run = h64::jadd2(run, bucket[b]);
        sum = h64::jadd2(sum, run);
      }
      win[w] = sum;
    }
  };
  const unsigned T = std::min<unsigned>(pick_threads(threads), W);
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker);
  worker();
  for (std::thread& th : pool) th.join();
  h64::Jac2 acc = h64::identity2();
  for (uint32_t w = W; w-- > 0;) {
    for (uint32_t s = 0; s < c; ++s) acc = h64::jdouble2(acc);
    acc = h64::jadd2(acc, win[w]);
  }
  const h64::Jac2 nrm = h64::normalise2(acc);
  std::memcpy(out192, &nrm, 192);
  return MSM_AMD_OK;
}

int msm_amd_host_msm_g2(int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
                        int threads, void* out192) {
  return host_msm_g2_entry(scalar_layout, g2_point_layout, scalars, points, n, threads, msm_amd::WidthBound{}, out192);
}

int msm_amd_host_msm_g2_bounded(int scalar_layout, int g2_point_layout, const void* scalars, const void* points, size_t n,
                                uint32_t bits, int sign, int threads, void* out192) {
  using namespace msm_amd;
  if (width_bound_check(bits, sign)) return MSM_AMD_INPUT_ERROR;
  WidthBound width;
  width.bits = bits, width.sign = (uint32_t)sign;
  return host_msm_g2_entry(scalar_layout, g2_point_layout, scalars, points, n, threads, width, out192);
}

// out[i] = start + i step (i < n), halo2curves G2Affine records (identity = all zero); threads over index ranges, one
// batched inversion per range.
int msm_amd_test_g2_progression(const void* start128, const void* step128, size_t n, int threads, void* out) {
  using namespace msm_amd;
  if (!start128 || !step128 || (n > 0 && !out)) return MSM_AMD_INPUT_ERROR;
  h64::Aff2 s0, st;
  std::memcpy(&s0, start128, 128);
  std::memcpy(&st, step128, 128);
  const h64::Jac2 stepj = h64::from_aff2(st);
  const unsigned T = (unsigned)std::max<size_t>(1, std::min<size_t>(pick_threads(threads), n / 1024 + 1));
  const size_t chunk = (n + T - 1) / T;
  auto worker = [&](unsigned t) {
    const size_t lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
    if (lo >= hi) return;
    // start + lo step by double-and-add
    h64::Jac2 cur = h64::identity2();
    for (int b = 63; b >= 0; --b) {
      cur = h64::jdouble2(cur);
      if ((lo >> b) & 1) cur = h64::jadd2(cur, stepj);
    }
    cur = h64::jadd2(cur, h64::from_aff2(s0));
    std::vector<h64::Jac2> pts(hi - lo);
    for (size_t i = lo; i < hi; ++i) {
      pts[i - lo] = cur;
      cur = h64::aff2_is_identity(st) ? cur : h64::jmadd2(cur, st);
    }
    // batched inversion of the z coordinates (identities skipped)
    std::vector<h64::Fe2> pref(hi - lo);
    h64::Fe2 run = h64::one2();
    for (size_t i = 0; i < pts.size(); ++i) {
      pref[i] = run;
      if (!h64::is_identity2(pts[i])) run = h64::mul2(run, pts[i].z);
    }
    h64::Fe2 inv = h64::inv2(run);
    uint8_t* o = (uint8_t*)out;
    for (size_t i = pts.size(); i-- > 0;) {
      h64::Aff2 a;
      if (h64::is_identity2(pts[i])) {
        std::memset(&a, 0, sizeof a);
      } else {
        const h64::Fe2 zi = h64::mul2(inv, pref[i]);
        inv = h64::mul2(inv, pts[i].z);
        const h64::Fe2 zi2 = h64::sqr2(zi);
        a.x = h64::mul2(pts[i].x, zi2);
        a.y = h64::mul2(pts[i].y, h64::mul2(zi2, zi));
      }
      std::memcpy(o + (lo + i) * 128, &a, 128);
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker, t);
  worker(0);
  for (std::thread& th : pool) th.join();
  return MSM_AMD_OK;
}

// Host twin of build_tables_g2_kernel: g2_table_walk per point on the CPU, entries as external affine records.
int msm_amd_test_g2_table_host(int g2_point_layout, const void* points, size_t n, uint32_t window_size,
                               uint32_t num_windows, int threads, void* out) {
  using namespace msm_amd;
  if (msm_amd_g2_point_bytes(g2_point_layout) == 0 || !points || !out || n == 0 || window_size == 0 ||
      window_size > 32 || num_windows == 0)
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* pt = (const uint8_t*)points;
  uint8_t* o = (uint8_t*)out;
  std::atomic<size_t> next{0};
  auto worker = [&]() {
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= n) break;
      h64::Aff2 raw;
      read_g2_point(g2_point_layout, pt, i, raw);
      Affine2 a;
      std::memcpy(&a, &raw, sizeof a);
      g2_table_walk(a, window_size, num_windows, [&](uint32_t w, const Aff2Packed& rec) {
        const Affine2 e = aff2packed_to_ext(rec);
        std::memcpy(o + ((size_t)w * n + i) * 128, &e, 128);
      });
    }
  };
  const unsigned T = (unsigned)std::min<size_t>(pick_threads(threads), n);
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker);
  worker();
  for (std::thread& th : pool) th.join();
  return MSM_AMD_OK;
}

int msm_amd_test_op_g2_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  using namespace msm_amd;
  if (op < 0 || (op >= G2RAW_OPS && op != MSM_AMD_G2_RAW_FQ2_SQRT) || (count > 0 && (!a || !b || !out)))
    return MSM_AMD_INPUT_ERROR;
  if (op == MSM_AMD_G2_RAW_FQ2_SQRT) {   // the root of the G2 decompression (compress_points.hip.h)
    for (size_t i = 0; i < count; ++i) raw_sqrt_fq2(a + i * kG2RawIn, out + i * kG2RawOut);
    return MSM_AMD_OK;
  }
  for (size_t i = 0; i < count; ++i) run_test_op_g2(op, a + i * kG2RawIn, b + i * kG2RawIn, out + i * kG2RawOut);
  return MSM_AMD_OK;
}

}  // extern "C"
