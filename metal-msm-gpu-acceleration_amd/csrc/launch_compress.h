// Launch wrappers of the compressed-point kernels (k_compress.hip) for the host driver (msm_host.hip), and the format
// rule the driver shares with the host twins (host_compress.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "compress_points.hip.h"

namespace msm_amd {

// counters: reset (launch_point_reset of launch_check.h)
// n compressed records (32 B, G2: 64 B) -> n records of `stride` bytes in an output layout; reasons: n bytes or nullptr
void launch_decompress(hipStream_t st, bool g2, int format, const void* in, uint32_t n, int layout, uint32_t stride,
                       void* out, uint8_t* reasons, PointCounters* counters);
// n affine records of `stride` bytes -> n compressed records; counters->by_reason[1] counts the all-0xFF records
void launch_compress(hipStream_t st, bool g2, int layout, uint32_t stride, const void* in, uint32_t n, int format, void* out,
                     PointCounters* counters);
// the root bodies at raw limbs: a = count x 36 (G2: 72) words, out = count x 40 (80) words
void launch_sqrt_raw(hipStream_t st, bool g2, const uint32_t* a, uint32_t* out, uint32_t count);

bool compress_format_known(int format);   // host_compress.hip

}  // namespace msm_amd
