// What the three units of the temporal reprojection share beside the gather's body (pt_temporal_gather.inc): pt_kernels_temporal.hip blends
// the gathered history with the current frame at once (include/mi355pt_temporal.h), pt_kernels_temporal_rectify.hip writes it to a scratch
// record per pixel and rectifies it against the current frame's local mean in a second launch (include/mi355pt_temporal_rectify.h),
// pt_kernels_temporal_flow.hip does either with a motion record per pixel (include/mi355pt_flow.h).  Device helpers, the record epilogue of
// the gather's body (the blend's stays spelled out in its kernels: as a function it changes their schedule), and the launch shape and template dispatch of the units' host launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

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

// the gather's epilogue: pixel p's scratch record, two 16-byte stores
static_assert(TEMPORAL_RECTIFY_RECORD_BYTES == 2 * sizeof(float4), "a scratch record is two float4");
__device__ __forceinline__ void tp_write_record(float4* record, size_t p, const float m1[3], const float m2[3], float L) {
    record[2 * p] = make_float4(m1[0], m1[1], m1[2], m2[0]);
    record[2 * p + 1] = make_float4(m2[1], m2[2], L, 0.0f);
}

// ---- host side: what every launcher of the three units starts with ----
// the launch shape of all their kernels, one thread per pixel; fills args.blocks_x, which the kernels find their block with
struct TpShape { dim3 grid, block; };
inline TpShape tp_shape(TemporalArgs& args) {
    args.blocks_x = (uint32_t)(((uint64_t)args.width + DN_BLOCK_X - 1) / DN_BLOCK_X);
    return TpShape{dim3(denoise_grid_blocks(args.width, args.height)), dim3(DN_BLOCK_X, DN_BLOCK_Y)};
}
// two run-time flags as a kernel's two bool template parameters: launch(std::bool_constant<b0>, std::bool_constant<b1>)
template <typename Launch>
void tp_dispatch(bool b0, bool b1, Launch&& launch) {
    if (b0 && b1) launch(std::true_type{}, std::true_type{});
    else if (b0) launch(std::true_type{}, std::false_type{});
    else if (b1) launch(std::false_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
}

}  // namespace

}  // namespace pt
