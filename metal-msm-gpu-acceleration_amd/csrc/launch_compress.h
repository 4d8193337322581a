// Launch wrappers of the compressed-point kernels (k_compress.hip) for the host driver (msm_host.hip), and the layout /
// report arithmetic the driver shares with the host twins (host_compress.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "compress_points.hip.h"

struct msm_amd_decompress_report;

namespace msm_amd {

// counters: zeroed, first_key all ones
void launch_compress_reset(hipStream_t st, CompressCounters* counters);
// n compressed records (32 B, G2: 64 B) -> n records of `stride` bytes in an output layout; reasons: n bytes or nullptr
void launch_decompress(hipStream_t st, bool g2, int format, const void* in, uint32_t n, int layout, uint32_t stride,
                       void* out, uint8_t* reasons, CompressCounters* counters);
// n affine records of `stride` bytes -> n compressed records; counters->by_reason[1] counts the all-0xFF records
void launch_compress(hipStream_t st, bool g2, int layout, uint32_t stride, const void* in, uint32_t n, int format, void* out,
                     CompressCounters* counters);
// the root bodies at raw limbs: a = count x 36 (G2: 72) words, out = count x 40 (80) words
void launch_sqrt_raw(hipStream_t st, bool g2, const uint32_t* a, uint32_t* out, uint32_t count);

// host_compress.hip: record size of an affine host layout of the group, of its prepared layout if `prepared_too`;
// 0 otherwise
size_t compress_stride(bool g2, int layout, bool prepared_too);
bool compress_format_known(int format);
void decompress_report_from_counters(const CompressCounters& c, size_t n, float device_ms, msm_amd_decompress_report* r);

}  // namespace msm_amd
