// What the two units of the temporal reprojection share beside the gather's body (pt_temporal_gather.inc): pt_kernels_temporal.hip blends
// the gathered history with the current frame at once (include/mi355pt_temporal.h), pt_kernels_temporal_rectify.hip writes it to a scratch
// record per pixel and rectifies it against the current frame's local mean in a second launch (include/mi355pt_temporal_rectify.h).
// Device helpers only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"

namespace pt {

namespace {

struct float3u { float x, y, z; };     // three consecutive words of a W x H x 3 film (12-byte records: no wider load is aligned)

__device__ __forceinline__ float3u tp_load3(const float* __restrict__ film, size_t pixel) {
    return float3u{film[3 * pixel], film[3 * pixel + 1], film[3 * pixel + 2]};
}
// an empty statement that takes the three values in registers and gives them back: what was loaded into them is loaded before it
__device__ __forceinline__ void tp_keep(float3u& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z)); }
__device__ __forceinline__ float tp_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

}  // namespace

}  // namespace pt
