// The bloom stage of include/mi355pt_bloom.h — bright pass, a pyramid of [1 3 3 1] reductions, bilinear expansions that mix the levels, the
// composite — as two HIP kernel templates for gfx950.  EXTENSION, no reference counterpart.  The shapes are bloom_plan.hpp's.
//
//   bloom_down_kernel<PREFILTER, FIREFLY>   level l -> l + 1.  A workgroup of 256 threads makes a tile of 32 x 8 destination pixels.  It stages
//                           the 66 x 18 source texels the tile reads — clamped coordinates, so every load is unconditional, all of a
//                           thread's loads issued before the first use — in LDS, one plane of floats per channel.  With PREFILTER the source
//                           is the film and a staged texel is cleaned, capped and bright-passed ONCE (a tap would do it up to 16 times), and
//                           with FIREFLY weighted, a fourth plane carrying the weight.  Then the horizontal pass, 18 rows x 32 columns into
//                           a second LDS array (two 8-byte reads per channel: lane i takes the texels 2 i .. 2 i + 3), then the vertical pass
//                           from it, one destination pixel per thread, and one 16-byte store.  A 32-lane half of a wave is one row of the
//                           tile in every phase, so no LDS access has a bank conflict (bloom_plan.hpp).
//   bloom_up_kernel<LAST>   level l + 1 -> l, one thread per destination pixel: four clamped, unconditional 16-byte loads of U_{l+1} and
//                           the thread's own D_l, which it overwrites with U_l.  LAST reads the film instead, and writes the 12-byte film
//                           pixel of the composite; film and out may be one buffer (neither is __restrict__; a thread reads its pixel
//                           before it writes it, and no other thread's result depends on that pixel).
//
// Every float operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls no
// fmaf), divisions are IEEE, there is no atomic operation: bit-equal to tests/bloom_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mi355pt_bloom.h"
#include "bloom_plan.hpp"
#include "launch.hpp"
#include "pt_denoise_common.hpp"

namespace pt {

namespace {

constexpr float BL_CAP = 4294967296.0f;      // 2^32: the cap on a cleaned value that enters the pyramid

__device__ __forceinline__ int bl_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <bool PREFILTER, bool FIREFLY>
__global__ __launch_bounds__(BLOOM_DOWN_BLOCK) void bloom_down_kernel(const void* __restrict__ src, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t tiles_x,
                                                                      BloomArgs a, const uint32_t* __restrict__ record, float4* __restrict__ dst) {
    static_assert(PREFILTER || !FIREFLY, "the weights belong to the first reduction");
    constexpr uint32_t C = FIREFLY ? 4u : 3u;
    constexpr uint32_t N_SRC = BLOOM_SRC_W * BLOOM_SRC_H, SRC_TRIPS = (N_SRC + BLOOM_DOWN_BLOCK - 1) / BLOOM_DOWN_BLOCK;
    constexpr uint32_t N_H = BLOOM_SRC_H * BLOOM_TX, H_TRIPS = (N_H + BLOOM_DOWN_BLOCK - 1) / BLOOM_DOWN_BLOCK;
    __shared__ __attribute__((aligned(16))) float s_src[C][BLOOM_SRC_H][BLOOM_SRC_PITCH];
    __shared__ float s_h[C][BLOOM_SRC_H][BLOOM_TX];
    const uint32_t tid = threadIdx.x;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x0 = 2 * (int)(tx * BLOOM_TX) - 1, y0 = 2 * (int)(ty * BLOOM_TY) - 1;

    // ---- the loads: SRC_TRIPS texels per thread at clamped coordinates (the last trip's surplus threads repeat the last texel) ----
    float v[SRC_TRIPS][3];
#pragma unroll
    for (uint32_t t = 0; t < SRC_TRIPS; ++t) {
        const uint32_t idx = min(t * BLOOM_DOWN_BLOCK + tid, N_SRC - 1u);
        const uint32_t sy = idx / BLOOM_SRC_W, sx = idx - sy * BLOOM_SRC_W;
        const uint64_t pix = (uint64_t)bl_clamp(y0 + (int)sy, (int)sh - 1) * sw + (uint32_t)bl_clamp(x0 + (int)sx, (int)sw - 1);
        if constexpr (PREFILTER) {
            const float* f = (const float*)src + 3 * pix;
            v[t][0] = f[0]; v[t][1] = f[1]; v[t][2] = f[2];
        } else {
            const float4 r = ((const float4*)src)[pix];
            v[t][0] = r.x; v[t][1] = r.y; v[t][2] = r.z;
        }
    }
    float T = 0.0f, k = 0.0f;
    if constexpr (PREFILTER) {
        const float E = record ? __uint_as_float(record[0]) : a.exposure;
        T = a.threshold / E;
        k = T * a.knee;
    }
    const float k2 = k + k, k4 = 4.0f * k;

    // ---- stage: with PREFILTER the clean, the cap, the bright pass and the weight, once per texel ----
#pragma unroll
    for (uint32_t t = 0; t < SRC_TRIPS; ++t) {
        const uint32_t idx = t * BLOOM_DOWN_BLOCK + tid;
        float p[4] = {v[t][0], v[t][1], v[t][2], 0.0f};
        if constexpr (PREFILTER) {
            float cc[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) cc[ch] = fminf(dn_clean(v[t][ch], a.spp), BL_CAP);
            const float m = fmaxf(fmaxf(cc[0], cc[1]), cc[2]);
            const float am = m - T;
            const float s = fminf(fmaxf(am + k, 0.0f), k2);
            const float q = k == 0.0f ? 0.0f : (s * s) / k4;
            const float g = fmaxf(q, am);
            const float f = m == 0.0f ? 0.0f : g / m;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) p[ch] = cc[ch] * f;
            if constexpr (FIREFLY) {
                const float Y = (0.2126f * p[0] + 0.7152f * p[1]) + 0.0722f * p[2];
                const float y1 = 1.0f + Y;
                const float w = 1.0f / y1;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) p[ch] = p[ch] * w;
                p[3] = w;
            }
        }
        if (idx < N_SRC) {
            const uint32_t sy = idx / BLOOM_SRC_W, sx = idx - sy * BLOOM_SRC_W;
#pragma unroll
            for (uint32_t ch = 0; ch < C; ++ch) s_src[ch][sy][sx] = p[ch];
        }
    }
    __syncthreads();

    // ---- the horizontal pass: row `row` of the staged texels, destination column i of the tile ----
#pragma unroll
    for (uint32_t t = 0; t < H_TRIPS; ++t) {
        const uint32_t item = t * BLOOM_DOWN_BLOCK + tid;
        if (item < N_H) {
            const uint32_t row = item / BLOOM_TX, i = item % BLOOM_TX;
#pragma unroll
            for (uint32_t ch = 0; ch < C; ++ch) {
                const float2 lo = *(const float2*)&s_src[ch][row][2u * i], hi = *(const float2*)&s_src[ch][row][2u * i + 2u];
                s_h[ch][row][i] = (lo.x + hi.y) + 3.0f * (lo.y + hi.x);
            }
        }
    }
    __syncthreads();

    // ---- the vertical pass: one destination pixel per thread ----
    const uint32_t ti = tid % BLOOM_TX, tj = tid / BLOOM_TX;
    float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t ch = 0; ch < C; ++ch) {
        const float h0 = s_h[ch][2u * tj][ti], h1 = s_h[ch][2u * tj + 1u][ti], h2 = s_h[ch][2u * tj + 2u][ti], h3 = s_h[ch][2u * tj + 3u][ti];
        const float vv = (h0 + h3) + 3.0f * (h1 + h2);
        r[ch] = vv * (1.0f / 64.0f);
    }
    if constexpr (FIREFLY) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) r[ch] = r[ch] / r[3];
    }
    const uint32_t i = tx * BLOOM_TX + ti, j = ty * BLOOM_TY + tj;
    if (i < dw && j < dh) dst[(uint64_t)j * dw + i] = make_float4(r[0], r[1], r[2], 0.0f);
}

// up: U_{l+1}, uw x uh.  The destination is dw x dh: level l in `lvl` (D_l in, U_l out) or, LAST, the frame (film in, out out)
template <bool LAST>
__global__ __launch_bounds__(BLOOM_UP_X* BLOOM_UP_Y) void bloom_up_kernel(const float4* __restrict__ up, uint32_t uw, uint32_t uh, uint32_t dw, uint32_t dh, uint32_t tiles_x,
                                                                          BloomArgs a, const float* film, float4* __restrict__ lvl, float* out) {
    const uint32_t tid = threadIdx.x;
    const uint32_t x = (blockIdx.x % tiles_x) * BLOOM_UP_X + tid % BLOOM_UP_X, y = (blockIdx.x / tiles_x) * BLOOM_UP_Y + tid / BLOOM_UP_X;
    const bool inside = x < dw && y < dh;
    const uint32_t xc = min(x, dw - 1u), yc = min(y, dh - 1u);      // a thread outside the level loads what its nearest pixel loads and stores nothing
    const int i = bl_clamp((int)(xc >> 1), (int)uw - 1), n = bl_clamp((xc & 1u) ? (int)(xc >> 1) + 1 : (int)(xc >> 1) - 1, (int)uw - 1);
    const int j = bl_clamp((int)(yc >> 1), (int)uh - 1), nj = bl_clamp((yc & 1u) ? (int)(yc >> 1) + 1 : (int)(yc >> 1) - 1, (int)uh - 1);
    const uint64_t pix = (uint64_t)yc * dw + xc;
    const float4 u00 = up[(uint64_t)j * uw + (uint32_t)i], u01 = up[(uint64_t)j * uw + (uint32_t)n];
    const float4 u10 = up[(uint64_t)nj * uw + (uint32_t)i], u11 = up[(uint64_t)nj * uw + (uint32_t)n];
    float own[3];
    if constexpr (LAST) {
        const float* f = film + 3 * pix;
        own[0] = f[0]; own[1] = f[1]; own[2] = f[2];
    } else {
        const float4 d = lvl[pix];
        own[0] = d.x; own[1] = d.y; own[2] = d.z;
    }
    const float a00[3] = {u00.x, u00.y, u00.z}, a01[3] = {u01.x, u01.y, u01.z}, a10[3] = {u10.x, u10.y, u10.z}, a11[3] = {u11.x, u11.y, u11.z};
    float o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float e0 = 3.0f * a00[ch] + a01[ch], e1 = 3.0f * a10[ch] + a11[ch];
        const float r = 3.0f * e0 + e1;
        const float X = r * (1.0f / 16.0f);
        if constexpr (LAST) o[ch] = (dn_clean(own[ch], a.spp) * a.base) + (X * a.intensity);
        else o[ch] = (own[ch] * a.s0) + (X * a.s1);
    }
    if (!inside) return;
    if constexpr (LAST) {
        float* q = out + 3 * pix;
        q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
    } else {
        lvl[pix] = make_float4(o[0], o[1], o[2], 0.0f);
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_bloom.cpp, which has checked every argument) ----
hipError_t launch_bloom(const float* d_film, const BloomArgs& args, const uint32_t* d_record, void* d_scratch, float* d_out, hipStream_t stream) {
    const BloomPlan plan = plan_bloom(args.width, args.height, args.levels);
    if (plan.levels == 0 || args.firefly > 1u) return hipErrorInvalidValue;      // a missing kernel is an error
    float4* const base = (float4*)d_scratch;
    const dim3 down_block(BLOOM_DOWN_BLOCK), up_block(BLOOM_UP_X * BLOOM_UP_Y);
    for (uint32_t l = 1; l <= plan.levels; ++l) {
        const BloomLevel &s = plan.level[l - 1], &d = plan.level[l];
        const uint32_t tiles_x = (d.width + BLOOM_TX - 1) / BLOOM_TX;
        const dim3 grid(d.down_blocks);
        if (l == 1 && args.firefly)
            hipLaunchKernelGGL((bloom_down_kernel<true, true>), grid, down_block, 0, stream, (const void*)d_film, s.width, s.height, d.width, d.height, tiles_x, args, d_record,
                               base + d.offset);
        else if (l == 1)
            hipLaunchKernelGGL((bloom_down_kernel<true, false>), grid, down_block, 0, stream, (const void*)d_film, s.width, s.height, d.width, d.height, tiles_x, args, d_record,
                               base + d.offset);
        else
            hipLaunchKernelGGL((bloom_down_kernel<false, false>), grid, down_block, 0, stream, (const void*)(base + s.offset), s.width, s.height, d.width, d.height, tiles_x, args,
                               d_record, base + d.offset);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (uint32_t l = plan.levels; l-- > 0;) {      // l = L - 1 .. 0: the size the launch writes
        const BloomLevel &u = plan.level[l + 1], &d = plan.level[l];
        const uint32_t tiles_x = (d.width + BLOOM_UP_X - 1) / BLOOM_UP_X;
        const dim3 grid(d.up_blocks);
        if (l == 0)
            hipLaunchKernelGGL((bloom_up_kernel<true>), grid, up_block, 0, stream, (const float4*)(base + u.offset), u.width, u.height, d.width, d.height, tiles_x, args, d_film,
                               (float4*)nullptr, d_out);
        else
            hipLaunchKernelGGL((bloom_up_kernel<false>), grid, up_block, 0, stream, (const float4*)(base + u.offset), u.width, u.height, d.width, d.height, tiles_x, args,
                               (const float*)nullptr, base + d.offset, (float*)nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
