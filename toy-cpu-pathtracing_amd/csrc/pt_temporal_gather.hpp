// What the units of the temporal reprojection share beside the gather itself (the body of temporal_kernel in pt_kernels_temporal.hip, which
// blends the gathered history with the current frame at once — include/mi355pt_temporal.h — or writes it to a scratch record per pixel
// that pt_kernels_temporal_rectify.hip rectifies against the current frame's local mean in a second launch —
// include/mi355pt_temporal_rectify.h).  Device helpers, the cleaned current values, the two store epilogues, and the launch shape and
// template dispatch of the units' host launchers.  pt_kernels_budget.hip and pt_kernels_upsample.hip take the device helpers too.
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

// the cleaned current values of pixel p: (c1, c2) with a half film, (c, 0) without
template <bool HAS_HALF>
__device__ __forceinline__ void tp_current(const TemporalFrameDev& cur, const TemporalArgs& a, size_t p, float c1[3], float c2[3]) {
    const float3u B = tp_load3(cur.film, p);
    c2[0] = 0.0f; c2[1] = 0.0f; c2[2] = 0.0f;
    if constexpr (HAS_HALF) {
        const float3u H = tp_load3(cur.half, p);
        c1[0] = dn_clean(H.x, a.half_spp); c1[1] = dn_clean(H.y, a.half_spp); c1[2] = dn_clean(H.z, a.half_spp);
        c2[0] = dn_clean(B.x - H.x, a.half_spp); c2[1] = dn_clean(B.y - H.y, a.half_spp); c2[2] = dn_clean(B.z - H.z, a.half_spp);
    } else {
        c1[0] = dn_clean(B.x, a.spp); c1[1] = dn_clean(B.y, a.spp); c1[2] = dn_clean(B.z, a.spp);
    }
}

// ---- the two store epilogues ----
// the blend's: pixel p of the accumulated films (out_half with a half film only) and of the history length
template <bool HAS_HALF>
__device__ __forceinline__ void tp_write_blend(float* __restrict__ out_film, float* __restrict__ out_half, float* __restrict__ out_length, size_t p,
                                               const float m1[3], const float m2[3], float L) {
    out_length[p] = L;
    if constexpr (HAS_HALF) {
        out_half[3 * p] = m1[0]; out_half[3 * p + 1] = m1[1]; out_half[3 * p + 2] = m1[2];
        out_film[3 * p] = m1[0] + m2[0]; out_film[3 * p + 1] = m1[1] + m2[1]; out_film[3 * p + 2] = m1[2] + m2[2];
    } else {
        out_film[3 * p] = m1[0]; out_film[3 * p + 1] = m1[1]; out_film[3 * p + 2] = m1[2];
    }
}
// the gather's: pixel p's scratch record, two 16-byte stores
static_assert(TEMPORAL_RECTIFY_RECORD_BYTES == 2 * sizeof(float4), "a scratch record is two float4");
__device__ __forceinline__ void tp_write_record(float4* record, size_t p, const float m1[3], const float m2[3], float L) {
    record[2 * p] = make_float4(m1[0], m1[1], m1[2], m2[0]);
    record[2 * p + 1] = make_float4(m2[1], m2[2], L, 0.0f);
}

// ---- host side: what the launchers of the temporal units start with ----
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
