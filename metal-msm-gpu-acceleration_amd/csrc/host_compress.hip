// Host twins of the compressed-point kernels (no ctx, no GPU): the bodies of compress_points.hip.h on the CPU, threaded
// over index ranges, and the layout / report arithmetic both the twins and the host driver (msm_host.hip) use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/msm_amd.h"
#include "launch_compress.h"

namespace msm_amd {

static_assert(kPointBadEncoding == MSM_AMD_POINT_BAD_ENCODING, "reason codes of compress_points.hip.h and msm_amd.h");
static_assert(kCompressedArk == MSM_AMD_COMPRESSED_ARK && kCompressedParity == MSM_AMD_COMPRESSED_PARITY, "formats");
static_assert(kLayoutPrepared == MSM_AMD_POINT_PREPARED && kG2LayoutH2cAffine == MSM_AMD_G2_POINT_H2C_AFFINE &&
                  kG2LayoutArkAffine == MSM_AMD_G2_POINT_ARK_AFFINE && kG2LayoutPrepared == MSM_AMD_G2_POINT_PREPARED,
              "layouts of compress_points.hip.h and msm_amd.h");
static_assert(sizeof(AffPacked) == 64 && sizeof(Aff2Packed) == MSM_AMD_G2_PREPARED_BYTES, "prepared record sizes");

bool compress_format_known(int format) { return format == MSM_AMD_COMPRESSED_ARK || format == MSM_AMD_COMPRESSED_PARITY; }

size_t compress_stride(bool g2, int layout, bool prepared_too) {
  if (g2) {
    if (layout == MSM_AMD_G2_POINT_H2C_AFFINE || layout == MSM_AMD_G2_POINT_ARK_AFFINE) return msm_amd_g2_point_bytes(layout);
    return prepared_too && layout == MSM_AMD_G2_POINT_PREPARED ? sizeof(Aff2Packed) : 0;
  }
  if (layout == MSM_AMD_POINT_H2C_AFFINE || layout == MSM_AMD_POINT_ARK_AFFINE) return msm_amd_point_bytes(layout);
  return prepared_too && layout == MSM_AMD_POINT_PREPARED ? sizeof(AffPacked) : 0;
}

void decompress_report_from_counters(const CompressCounters& c, size_t n, float device_ms, msm_amd_decompress_report* r) {
  *r = msm_amd_decompress_report{};
  r->n_checked = n;
  for (int k = 0; k < 5; ++k) r->by_reason[k] = c.by_reason[k];
  r->n_invalid = (uint64_t)c.by_reason[1] + c.by_reason[2] + c.by_reason[3] + c.by_reason[4];
  r->n_identity = c.n_identity;
  const bool none = c.first_key == ~0ull;
  r->first_invalid = none ? UINT64_MAX : (c.first_key >> 3);
  r->first_reason = none ? 0u : (uint32_t)(c.first_key & 7u);
  r->device_ms = device_ms;
}

namespace {

unsigned worker_count(int threads, size_t n) {
  const unsigned want = threads > 0 ? (unsigned)threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  return (unsigned)std::max<size_t>(1, std::min<size_t>(want, n));
}

// fn(t, lo, hi) on T threads over [0, n)
template <typename F>
void for_ranges(unsigned T, size_t n, F fn) {
  const size_t chunk = (n + T - 1) / T;
  auto worker = [&](unsigned t) {
    const size_t lo = std::min(n, t * chunk), hi = std::min(n, lo + chunk);
    fn(t, lo, hi);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < T; ++t) pool.emplace_back(worker, t);
  worker(0);
  for (std::thread& th : pool) th.join();
}

int host_decompress(bool g2, int format, const void* in_v, size_t n, int layout, int threads, void* out_v,
                    uint8_t* reasons, msm_amd_decompress_report* report) {
  const size_t stride = compress_stride(g2, layout, false);
  if (!report || stride == 0 || !compress_format_known(format) || n > 0xFFFFFFFFull || (n > 0 && (!in_v || !out_v)))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const unsigned T = worker_count(threads, n);
  std::vector<CompressCounters> part(T);
  for_ranges(T, n, [&](unsigned t, size_t lo, size_t hi) {
    CompressCounters c{};
    c.first_key = ~0ull;
    for (size_t i = lo; i < hi; ++i) {
      bool identity = false;
      uint32_t reason;
      if (g2) {
        Aff2I pt;
        reason = decompress_record_g2(format, in + i * 64, pt, identity);
        decompress_store_g2(layout, out + i * stride, pt);
      } else {
        AffI pt;
        reason = decompress_record_g1(format, in + i * 32, pt, identity);
        decompress_store_g1(layout, out + i * stride, pt);
      }
      if (reasons) reasons[i] = (uint8_t)reason;
      ++c.by_reason[reason];
      c.n_identity += identity;
      if (reason != kPointValid) c.first_key = std::min<uint64_t>(c.first_key, ((uint64_t)i << 3) | reason);
    }
    part[t] = c;
  });
  CompressCounters sum{};
  sum.first_key = ~0ull;
  for (const CompressCounters& c : part) {
    for (int k = 0; k < 5; ++k) sum.by_reason[k] += c.by_reason[k];
    sum.n_identity += c.n_identity;
    sum.first_key = std::min(sum.first_key, c.first_key);
  }
  decompress_report_from_counters(sum, n, 0.0f, report);
  return MSM_AMD_OK;
}

int host_compress(bool g2, int layout, const void* in_v, size_t n, int format, int threads, void* out_v, uint64_t* n_bad) {
  const size_t stride = compress_stride(g2, layout, false);
  if (stride == 0 || !compress_format_known(format) || n > 0xFFFFFFFFull || (n > 0 && (!in_v || !out_v)))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const unsigned T = worker_count(threads, n);
  std::vector<uint64_t> part(T, 0);
  for_ranges(T, n, [&](unsigned t, size_t lo, size_t hi) {
    uint64_t bad = 0;
    for (size_t i = lo; i < hi; ++i)
      bad += g2 ? compress_record_g2(layout, in + i * stride, format, out + i * 64)
                : compress_record_g1(layout, in + i * stride, format, out + i * 32);
    part[t] = bad;
  });
  uint64_t bad = 0;
  for (uint64_t b : part) bad += b;
  if (n_bad) *n_bad = bad;
  return MSM_AMD_OK;
}

}  // namespace
}  // namespace msm_amd

extern "C" {

size_t msm_amd_compressed_bytes(int format, int group) {
  if (!msm_amd::compress_format_known(format)) return 0;
  return group == 1 ? 32 : group == 2 ? 64 : 0;
}

int msm_amd_host_decompress_points(int format, const void* in, size_t n, int point_layout_out, int threads, void* out,
                                   uint8_t* reasons, msm_amd_decompress_report* report) {
  return msm_amd::host_decompress(false, format, in, n, point_layout_out, threads, out, reasons, report);
}

int msm_amd_host_g2_decompress_points(int format, const void* in, size_t n, int g2_point_layout_out, int threads,
                                      void* out, uint8_t* reasons, msm_amd_decompress_report* report) {
  return msm_amd::host_decompress(true, format, in, n, g2_point_layout_out, threads, out, reasons, report);
}

int msm_amd_host_compress_points(int point_layout_in, const void* in, size_t n, int format, int threads, void* out,
                                 uint64_t* n_bad) {
  return msm_amd::host_compress(false, point_layout_in, in, n, format, threads, out, n_bad);
}

int msm_amd_host_g2_compress_points(int g2_point_layout_in, const void* in, size_t n, int format, int threads, void* out,
                                    uint64_t* n_bad) {
  return msm_amd::host_compress(true, g2_point_layout_in, in, n, format, threads, out, n_bad);
}

}  // extern "C"
