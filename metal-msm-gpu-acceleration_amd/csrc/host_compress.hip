// Host twins of the compressed-point kernels (no ctx, no GPU): the bodies of compress_points.hip.h on the CPU, threaded
// over index ranges; the report is the counter fold of point_report.hip.h.
#include <hip/hip_runtime.h>

#include "../../include/msm_amd.h"
#include "host_threads.h"
#include "launch_compress.h"

namespace msm_amd {

static_assert(kCompressedArk == MSM_AMD_COMPRESSED_ARK && kCompressedParity == MSM_AMD_COMPRESSED_PARITY, "formats");
static_assert(sizeof(AffPacked) == 64 && sizeof(Aff2Packed) == MSM_AMD_G2_PREPARED_BYTES, "prepared record sizes");

bool compress_format_known(int format) { return format == MSM_AMD_COMPRESSED_ARK || format == MSM_AMD_COMPRESSED_PARITY; }

namespace {

int host_decompress(bool g2, int format, const void* in_v, size_t n, int layout, int threads, void* out_v,
                    uint8_t* reasons, msm_amd_decompress_report* report) {
  const size_t stride = point_record_bytes(g2, layout, kKindAffine);
  if (!report || stride == 0 || !compress_format_known(format) || n > 0xFFFFFFFFull || (n > 0 && (!in_v || !out_v)))
    return MSM_AMD_INPUT_ERROR;
  const uint8_t* in = (const uint8_t*)in_v;
  uint8_t* out = (uint8_t*)out_v;
  const unsigned T = worker_count(threads, n);
  std::vector<PointCounters> part(T);
  for_ranges(T, n, [&](unsigned t, size_t lo, size_t hi) {
    PointCounters c = point_counters_empty();
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
      point_counters_add(c, i, reason, identity);
    }
    part[t] = c;
  });
  PointCounters sum = point_counters_empty();
  for (const PointCounters& c : part) point_counters_merge(sum, c);
  point_report_decode(sum, n, 0.0f, report);
  return MSM_AMD_OK;
}

int host_compress(bool g2, int layout, const void* in_v, size_t n, int format, int threads, void* out_v, uint64_t* n_bad) {
  const size_t stride = point_record_bytes(g2, layout, kKindAffine);
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
