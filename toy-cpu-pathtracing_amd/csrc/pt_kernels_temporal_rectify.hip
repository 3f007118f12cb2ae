// The rectified temporal accumulation of include/mi355pt_temporal_rectify.h as two HIP kernels for gfx950.  EXTENSION, no reference
// counterpart.  Both run one thread per pixel on the grid of the temporal unit (64 x 4 blocks), without atomics and without scratch memory.
//
// 1. pt_kernels_temporal.hip's temporal_kernel<.., RECORD = true>: the gather of the accumulation with another epilogue: instead of
//    blending it writes hist1, hist2 (hist, 0 without a half film) and "L, or 0 without history" as one 32-byte record per pixel — two
//    16-byte stores — into the caller's scratch.  It does not read the current film.
// 2. temporal_rectify_kernel, this unit: an LDS stencil.  A workgroup loads its 64 x 4 tile plus an apron of RADIUS pixels (indices clamped to the
//    frame; a pixel outside it is no member) and keeps per tile pixel the cleaned current value v, the history mean g (both 0 for a
//    non-member) and the membership flag as PLANES of (64 + 2 RADIUS) x (4 + 2 RADIUS) words: the 64 lanes of a wave then read consecutive
//    words at every window offset.  After the barrier each thread forms the window sums in the header's order — row sums left to right
//    from 0, then the row sums top to bottom from 0 — from LDS alone, computes k, and blends its own pixel, whose c and hist it reads once
//    more from the current films and the scratch (lines its workgroup has just loaded).
//
// Every operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls no
// fmaf), division and sqrtf are IEEE (hipcc's default: correctly rounded, no fast-math): the result is bit-equal to
// tests/temporal_rectify_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

constexpr int TR_PLANES = 7;       // v.x v.y v.z  g.x g.y g.z  member

template <bool HAS_HALF, int RADIUS>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_rectify_kernel(TemporalFrameDev cur, TemporalArgs a, float gamma,
                                                                                   const float4* __restrict__ record, float* __restrict__ out_film,
                                                                                   float* __restrict__ out_half, float* __restrict__ out_length) {
    constexpr int TW = DN_BLOCK_X + 2 * RADIUS, TH = DN_BLOCK_Y + 2 * RADIUS, TN = TW * TH, THREADS = DN_BLOCK_X * DN_BLOCK_Y;
    __shared__ float tile[TR_PLANES][TN];

    const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
    const int wm1 = (int)a.width - 1, hm1 = (int)a.height - 1;
    const int ox = (int)(bx * DN_BLOCK_X) - RADIUS, oy = (int)(by * DN_BLOCK_Y) - RADIUS;
    // the tile and its apron: every load at an index clamped to the frame
    for (int i = (int)(threadIdx.y * DN_BLOCK_X + threadIdx.x); i < TN; i += THREADS) {
        const int ty = i / TW, tx = i - ty * TW;
        const int qx = ox + tx, qy = oy + ty;
        const bool inside = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
        const int cx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
        const size_t q = (size_t)cy * a.width + (size_t)cx;
        const float4 ra = record[2 * q], rb = record[2 * q + 1];
        float c1[3], c2[3];
        tp_current<HAS_HALF>(cur, a, q, c1, c2);
        const bool member = inside && rb.z > 0.0f;
        const float h1[3] = {ra.x, ra.y, ra.z}, h2[3] = {ra.w, rb.x, rb.y};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = HAS_HALF ? (c1[ch] + c2[ch]) * 0.5f : c1[ch];
            const float g = HAS_HALF ? (h1[ch] + h2[ch]) * 0.5f : h1[ch];
            tile[ch][i] = member ? v : 0.0f;
            tile[3 + ch][i] = member ? g : 0.0f;
        }
        tile[6][i] = member ? 1.0f : 0.0f;
    }
    __syncthreads();

    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    // the pixel's own values
    const float4 ra = record[2 * p], rb = record[2 * p + 1];
    float c1[3], c2[3];
    tp_current<HAS_HALF>(cur, a, p, c1, c2);
    const float h1[3] = {ra.x, ra.y, ra.z}, h2[3] = {ra.w, rb.x, rb.y};
    const bool has = rb.z > 0.0f;
    const float alpha = 1.0f / rb.z;

    // the window sums: row sums first, each from 0, then the row sums from 0
    float S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f}, Sg[3] = {0.0f, 0.0f, 0.0f}, n = 0.0f;
#pragma unroll
    for (int dy = 0; dy <= 2 * RADIUS; ++dy) {
        float r1[3] = {0.0f, 0.0f, 0.0f}, r2[3] = {0.0f, 0.0f, 0.0f}, rg[3] = {0.0f, 0.0f, 0.0f}, rn = 0.0f;
#pragma unroll
        for (int dx = 0; dx <= 2 * RADIUS; ++dx) {
            const int i = ((int)threadIdx.y + dy) * TW + (int)threadIdx.x + dx;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float v = tile[ch][i];
                r1[ch] = r1[ch] + v;
                r2[ch] = r2[ch] + v * v;
                rg[ch] = rg[ch] + tile[3 + ch][i];
            }
            rn = rn + tile[6][i];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            S1[ch] = S1[ch] + r1[ch];
            S2[ch] = S2[ch] + r2[ch];
            Sg[ch] = Sg[ch] + rg[ch];
        }
        n = n + rn;
    }

    float m1[3], m2[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float mu = S1[ch] / n;
        const float d = S2[ch] / n - mu * mu;
        const float s2 = d > 0.0f ? d : 0.0f;
        const float se = sqrtf(s2 / n);
        const float muh = Sg[ch] / n;
        const float lo = mu - gamma * se, hi = mu + gamma * se;
        const float tgt = fminf(fmaxf(muh, lo), hi);
        const float k = muh > 0.0f ? tgt / muh : 1.0f;
        const float r1 = h1[ch] * k;
        const float b1 = r1 + (c1[ch] - r1) * alpha;
        m1[ch] = has ? b1 : c1[ch];
        if constexpr (HAS_HALF) {
            const float r2 = h2[ch] * k;
            const float b2 = r2 + (c2[ch] - r2) * alpha;
            m2[ch] = has ? b2 : c2[ch];
        }
    }

    tp_write_blend<HAS_HALF>(out_film, out_half, out_length, p, m1, m2, has ? rb.z : 1.0f);
}

template <bool HAS_HALF>
void launch_rectify_radius(uint32_t radius, const TpShape& sh, hipStream_t stream, const TemporalFrameDev& cur, const TemporalArgs& args, float gamma,
                           const float4* record, float* d_out_film, float* d_out_half, float* d_out_length) {
#define PT_TR_LAUNCH(R) \
    hipLaunchKernelGGL((temporal_rectify_kernel<HAS_HALF, R>), sh.grid, sh.block, 0, stream, cur, args, gamma, record, d_out_film, d_out_half, d_out_length)
    if (radius == 1) PT_TR_LAUNCH(1);
    else if (radius == 2) PT_TR_LAUNCH(2);
    else PT_TR_LAUNCH(3);
#undef PT_TR_LAUNCH
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_temporal.cpp's driver, which has checked every argument) ----
// the second launch of every rectified form, over the records launch_temporal_gather has written
hipError_t launch_temporal_rectify_blend(const TemporalFrameDev& cur, TemporalArgs args, uint32_t radius, float gamma, const void* d_scratch, float* d_out_film,
                                         float* d_out_half, float* d_out_length, hipStream_t stream) {
    if (radius < 1 || radius > 3) return hipErrorInvalidValue;
    const TpShape sh = tp_shape(args);
    const float4* record = (const float4*)d_scratch;
    if (cur.half != nullptr) launch_rectify_radius<true>(radius, sh, stream, cur, args, gamma, record, d_out_film, d_out_half, d_out_length);
    else launch_rectify_radius<false>(radius, sh, stream, cur, args, gamma, record, d_out_film, d_out_half, d_out_length);
    return hipGetLastError();
}

}  // namespace pt
