// The sample budget by reprojected history (include/mi355pt_budget.h, which is normative for the arithmetic and its order): wave64 kernels
// for gfx950.  EXTENSION, no reference counterpart.
//   budget_probe_kernel<CARRY, HAS_PREV_IDS>   the GEOMETRIC half of the temporal gather (the body of temporal_kernel in
//                            pt_kernels_temporal.hip, restated here without the films — text of its own, because with the shared part
//                            as functions the probe lost one to three waves per SIMD): one wave per 8x8 tile, lane =
//                            pixel (lane & 7, lane >> 3) of the tile — adaptive_err_kernel's mapping —, four tiles per 256-thread block,
//                            grid-stride over the tiles.  Per lane the projection and four clamped, unconditional tap loads of hit.y,
//                            length, position and shading_normal (with ids also the id): no film or half loads at all.  A lane outside
//                            the frame runs the clamped pixel of the frame's edge and is selected away.  Validity is decided by selects
//                            on loaded values: a branch the compiler forms stands around arithmetic only, never around a load.  The
//                            tile's minimum is a xor butterfly over 32, 16, .. 1 lanes (fminf of values that are >= 0 or +inf commutes
//                            and associates: every lane holds the minimum); lane 0 writes the tile's two words.  CARRY, as
//                            TemporalCarryDev::kind: 0 the static world, 1 the per-instance table (mi355pt_motion.h), 2 the per-pixel
//                            records (mi355pt_flow.h).
//   budget_fill_kernel       the probe without a previous frame: every P is 0, every tile gets budget_spp(0); no G-buffer is read.
//   budget_select_kernel     one wave per tile: the flag "clamped tile_spp > level" for adaptive_compact_kernel, and H := F on the flagged
//                            tiles' in-frame pixels — the copy adaptive_err_kernel does for its active tiles.
//   pair_normalize_tiles_kernel, length_credit_kernel   streaming, one thread per pixel.
// No LDS, no atomics, no scratch memory.  Every operation is a single binary32 operation in the order the headers state (the unit is built
// with -ffp-contract=off and calls no fmaf), divisions are IEEE: the result is bit-equal to tests/budget_reference.py, and P to what the
// accumulation kernels gather on the same inputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "budget_plan.hpp"
#include "launch.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

constexpr uint32_t BG_BLOCK = 256, BG_TILES_PER_BLOCK = BG_BLOCK / 64;

template <int CARRY, bool HAS_PREV_IDS>
__global__ __launch_bounds__(BG_BLOCK) void budget_probe_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a, TemporalCarryDev cv, BudgetTilesDev bt,
                                                                float* __restrict__ pred, float* __restrict__ tile_len, uint32_t* __restrict__ tile_spp) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int wm1 = (int)a.width - 1, hm1 = (int)a.height - 1;
    for (uint32_t tile = blockIdx.x * BG_TILES_PER_BLOCK + wave; tile < bt.n_tiles; tile += gridDim.x * BG_TILES_PER_BLOCK) {
        const uint32_t tx = tile % bt.tiles_x, ty = tile / bt.tiles_x;
        const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
        const bool in = px < a.width && py < a.height;
        // a lane outside the frame reads the frame's edge pixel: every load below is in bounds, and `in` selects its value away
        const size_t p = (size_t)(py < a.height ? py : a.height - 1u) * a.width + (px < a.width ? px : a.width - 1u);

        // geometry of p, as the gather's (h == 0 makes NaNs and infinities: `ok` selects them away)
        uint32_t idc = 0u;
        float4 r0, r1, r2, r3, r4, r5;
        if constexpr (CARRY == 2) {
            const float4* const frec = (const float4*)(cv.flow + p);
            r0 = frec[0]; r1 = frec[1];
            if constexpr (HAS_PREV_IDS) idc = cv.ids_cur[p];
        } else if constexpr (CARRY == 1) {
            idc = cv.ids_cur[p];
            const float4* const mrec = (const float4*)(cv.table + (idc < cv.last_entry ? idc : cv.last_entry));
            r0 = mrec[0]; r1 = mrec[1]; r2 = mrec[2]; r3 = mrec[3]; r4 = mrec[4]; r5 = mrec[5];
        }
        const float3u P = tp_load3(cur.position, p), N = tp_load3(cur.shading_normal, p);
        const float hx = cur.hit[3 * p], h = cur.hit[3 * p + 1];
        float Xx, Xy, Xz, nx, ny, nz;
        if constexpr (CARRY == 2) {
            Xx = P.x / h + r0.x; Xy = P.y / h + r0.y; Xz = P.z / h + r0.z;                                           // Xp = X + d
            nx = (2.0f * (N.x / h) - 1.0f) + r1.x; ny = (2.0f * (N.y / h) - 1.0f) + r1.y; nz = (2.0f * (N.z / h) - 1.0f) + r1.z;
        } else if constexpr (CARRY == 1) {
            // a = r0.xyzw r1.xyzw r2.x,  b = r2.yzw,  n = r3.xyzw r4.xyzw r5.x: Xp = a X + b, nrm = n nrm
            const float X0 = P.x / h, X1 = P.y / h, X2 = P.z / h;
            Xx = tp_dot(r0.x, r0.y, r0.z, X0, X1, X2) + r2.y; Xy = tp_dot(r0.w, r1.x, r1.y, X0, X1, X2) + r2.z;
            Xz = tp_dot(r1.z, r1.w, r2.x, X0, X1, X2) + r2.w;
            const float n0 = 2.0f * (N.x / h) - 1.0f, n1 = 2.0f * (N.y / h) - 1.0f, n2 = 2.0f * (N.z / h) - 1.0f;
            nx = tp_dot(r3.x, r3.y, r3.z, n0, n1, n2); ny = tp_dot(r3.w, r4.x, r4.y, n0, n1, n2); nz = tp_dot(r4.z, r4.w, r5.x, n0, n1, n2);
        } else {
            Xx = P.x / h + a.delta[0]; Xy = P.y / h + a.delta[1]; Xz = P.z / h + a.delta[2];                        // Xp = X + delta
            nx = 2.0f * (N.x / h) - 1.0f; ny = 2.0f * (N.y / h) - 1.0f; nz = 2.0f * (N.z / h) - 1.0f;
        }
        const float t = hx / h;
        // projection into the previous image
        const float vx = tp_dot(a.rows[0], a.rows[1], a.rows[2], Xx, Xy, Xz);
        const float vy = tp_dot(a.rows[3], a.rows[4], a.rows[5], Xx, Xy, Xz);
        const float zc = -tp_dot(a.rows[6], a.rows[7], a.rows[8], Xx, Xy, Xz);
        const float gx = (a.cx + (vx / zc) * a.sx) - 0.5f, gy = (a.cy - (vy / zc) * a.sy) - 0.5f;
        const bool ok = h != 0.0f && zc > 0.0f && gx >= -1.0f && gx < a.wf && gy >= -1.0f && gy < a.hf;
        const float gxs = ok ? gx : 0.0f, gys = ok ? gy : 0.0f;           // (a finite value in [-1, W): the conversions below are defined)
        const float x0f = floorf(gxs), y0f = floorf(gys);
        const float wx = gxs - x0f, wy = gys - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;                           // -1 .. W - 1, -1 .. H - 1
        const float omx = 1.0f - wx, omy = 1.0f - wy;
        const float bw[4] = {omx * omy, wx * omy, omx * wy, wx * wy};
        const float tol = a.pos_tol * t;

        // the four taps: every load at an index clamped to the frame, issued whatever `ok` and the tap's validity are
        float w[4], len[4], hq[4];
        bool inside[4];
        uint32_t idq[4] = {0u, 0u, 0u, 0u};      // the taps' ids (read with the previous frame's ids only)
        float3u Pq[4], Nq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            inside[k] = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
            const int cqx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cqy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
            const size_t q = (size_t)cqy * a.width + (size_t)cqx;
            hq[k] = prev.hit[3 * q + 1];
            len[k] = prev.length[q];
            Pq[k] = tp_load3(prev.position, q); Nq[k] = tp_load3(prev.shading_normal, q);
            if constexpr (CARRY != 0 && HAS_PREV_IDS) idq[k] = cv.ids_prev[q];
        }
        // A tap's values are needed only where the tests before them pass, and the compiler would sink their loads into a branch on that
        // (it turns a select whose operand is a load into control flow).  As the gather's tp_keep: the loaded values are pinned here, after
        // all four taps' loads have been issued
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tp_keep(Pq[k]); tp_keep(Nq[k]);
            asm volatile("" : "+v"(hq[k]), "+v"(len[k]));
            if constexpr (CARRY != 0 && HAS_PREV_IDS) asm volatile("" : "+v"(idq[k]));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ex = Xx - Pq[k].x / hq[k], ey = Xy - Pq[k].y / hq[k], ez = Xz - Pq[k].z / hq[k];
            const float pd = fabsf(tp_dot(ex, ey, ez, nx, ny, nz));
            const float qnx = 2.0f * (Nq[k].x / hq[k]) - 1.0f, qny = 2.0f * (Nq[k].y / hq[k]) - 1.0f, qnz = 2.0f * (Nq[k].z / hq[k]) - 1.0f;
            const float nd = tp_dot(nx, ny, nz, qnx, qny, qnz);
            const bool same = !(CARRY != 0 && HAS_PREV_IDS) || idq[k] == idc;      // the tap shows the pixel's instance (always, without the previous frame's ids)
            const bool valid = ok && inside[k] && hq[k] > 0.0f && len[k] > 0.0f && pd <= tol && nd >= a.normal_cos && same;
            w[k] = valid ? bw[k] : 0.0f;
            len[k] = valid ? len[k] : 0.0f;
        }
        const float Wt = ((w[0] + w[1]) + w[2]) + w[3];
        const bool has = Wt > a.min_weight;
        const float Lh = (((w[0] * len[0] + w[1] * len[1]) + w[2] * len[2]) + w[3] * len[3]) / Wt;
        const float Pl = has ? Lh : 0.0f;
        if (pred != nullptr && in) pred[(size_t)py * a.width + px] = Pl;

        // the tile's minimum: a P that is not > 0 counts as 0, a lane outside the frame as +inf (the tile's first pixel is inside)
        float v = in ? (Pl > 0.0f ? Pl : 0.0f) : INFINITY;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
        if (lane == 0) {
            tile_len[tile] = v;
            tile_spp[tile] = budget_spp(v, bt.base_spp, bt.max_spp, bt.target_history);
        }
    }
}

__global__ __launch_bounds__(256) void budget_fill_kernel(uint32_t width, uint32_t height, BudgetTilesDev bt, float* __restrict__ pred,
                                                          float* __restrict__ tile_len, uint32_t* __restrict__ tile_spp) {
    const size_t n_pix = (size_t)width * height, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pred != nullptr)
        for (size_t i = first; i < n_pix; i += stride) pred[i] = 0.0f;
    const uint32_t n = budget_spp(0.0f, bt.base_spp, bt.max_spp, bt.target_history);
    for (size_t t = first; t < bt.n_tiles; t += stride) { tile_len[t] = 0.0f; tile_spp[t] = n; }
}

__global__ __launch_bounds__(BG_BLOCK) void budget_select_kernel(const float* __restrict__ film, float* __restrict__ half, uint32_t width, uint32_t height,
                                                                 uint32_t tiles_x, uint32_t n_tiles, const uint32_t* __restrict__ tile_spp,
                                                                 uint32_t* __restrict__ flags, uint32_t level_spp, uint32_t base_spp, uint32_t max_spp) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x * BG_TILES_PER_BLOCK + wave; tile < n_tiles; tile += gridDim.x * BG_TILES_PER_BLOCK) {
        const bool flagged = budget_clamp(tile_spp[tile], base_spp, max_spp) > level_spp;        // wave-uniform
        if (lane == 0) flags[tile] = flagged ? 1u : 0u;
        if (!flagged) continue;
        const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
        const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
        if (px < width && py < height) {
            const size_t o = ((size_t)py * width + px) * 3u;
            half[o] = film[o]; half[o + 1] = film[o + 1]; half[o + 2] = film[o + 2];
        }
    }
}

__global__ __launch_bounds__(256) void pair_normalize_tiles_kernel(const float* film, const float* half, const uint32_t* __restrict__ tile_spp, uint32_t width,
                                                                   uint32_t height, uint32_t tiles_x, float* out_film, float* out_half) {     // (in place allowed)
    const size_t n_pix = (size_t)width * height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t px = (uint32_t)(i % width), py = (uint32_t)(i / width);
        const float n = (float)(tile_spp[(py >> 3) * tiles_x + (px >> 3)] / 2u);
        const float f0 = film[3 * i], f1 = film[3 * i + 1], f2 = film[3 * i + 2], h0 = half[3 * i], h1 = half[3 * i + 1], h2 = half[3 * i + 2];
        out_film[3 * i] = f0 / n; out_film[3 * i + 1] = f1 / n; out_film[3 * i + 2] = f2 / n;
        out_half[3 * i] = h0 / n; out_half[3 * i + 1] = h1 / n; out_half[3 * i + 2] = h2 / n;
    }
}

__global__ __launch_bounds__(256) void length_credit_kernel(float* __restrict__ length, const uint32_t* __restrict__ tile_spp, uint32_t base_spp, float max_history,
                                                            uint32_t width, uint32_t height, uint32_t tiles_x) {
    const size_t n_pix = (size_t)width * height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t px = (uint32_t)(i % width), py = (uint32_t)(i / width);
        const uint32_t n = tile_spp[(py >> 3) * tiles_x + (px >> 3)];
        if (n > base_spp) length[i] = fminf(length[i] + (float)(n / base_spp - 1u), max_history);
    }
}

uint32_t tile_grid(uint32_t n_tiles) { return std::min<uint32_t>((n_tiles + BG_TILES_PER_BLOCK - 1u) / BG_TILES_PER_BLOCK, 8192u); }
uint32_t pixel_grid(uint32_t width, uint32_t height) { return (uint32_t)std::min<size_t>(((size_t)width * height + 255u) / 256u, 4096u); }

}  // namespace

// ---- host side (declared in launch.hpp; called from api_budget.cpp, which has checked every argument) ----
hipError_t launch_budget_probe(const TemporalFrameDev& cur, const TemporalFrameDev* prev, TemporalArgs args, const TemporalCarryDev& carry, BudgetTilesDev tiles,
                               float* d_pred, float* d_tile_len, uint32_t* d_tile_spp, hipStream_t stream) {
    tiles.n_tiles = adaptive_tile_count(args.width, args.height);
    tiles.tiles_x = (args.width + 7u) / 8u;
    if (tiles.n_tiles == 0u) return hipErrorInvalidValue;
    if (!prev) {
        hipLaunchKernelGGL(budget_fill_kernel, dim3(pixel_grid(args.width, args.height)), dim3(256), 0, stream, args.width, args.height, tiles, d_pred, d_tile_len,
                           d_tile_spp);
        return hipGetLastError();
    }
    const dim3 grid(tile_grid(tiles.n_tiles)), block(BG_BLOCK);
    const bool ids = carry.ids_prev != nullptr;
#define PT_BG_LAUNCH(CARRY, IDS) \
    hipLaunchKernelGGL((budget_probe_kernel<CARRY, IDS>), grid, block, 0, stream, cur, *prev, args, carry, tiles, d_pred, d_tile_len, d_tile_spp)
    if (carry.kind == CARRY_FLOW) { if (ids) PT_BG_LAUNCH(CARRY_FLOW, true); else PT_BG_LAUNCH(CARRY_FLOW, false); }
    else if (carry.kind == CARRY_TABLE) { if (ids) PT_BG_LAUNCH(CARRY_TABLE, true); else PT_BG_LAUNCH(CARRY_TABLE, false); }
    else PT_BG_LAUNCH(CARRY_STATIC, false);
#undef PT_BG_LAUNCH
    return hipGetLastError();
}

hipError_t launch_budget_select(const float* d_film, float* d_half, uint32_t width, uint32_t height, const uint32_t* d_tile_spp, uint32_t level_spp,
                                uint32_t base_spp, uint32_t max_spp, void* d_scratch, uint32_t* d_list, uint32_t* d_count, hipStream_t stream) {
    const uint32_t n_tiles = adaptive_tile_count(width, height);
    if (n_tiles == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(budget_select_kernel, dim3(tile_grid(n_tiles)), dim3(BG_BLOCK), 0, stream, d_film, d_half, width, height, (width + 7u) / 8u, n_tiles,
                       d_tile_spp, (uint32_t*)d_scratch, level_spp, base_spp, max_spp);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_adaptive_compact((const uint32_t*)d_scratch, n_tiles, d_list, d_count, stream);
}

hipError_t launch_pair_normalize_tiles(const float* d_film, const float* d_half, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_out_film,
                                       float* d_out_half, hipStream_t stream) {
    if (adaptive_tile_count(width, height) == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pair_normalize_tiles_kernel, dim3(pixel_grid(width, height)), dim3(256), 0, stream, d_film, d_half, d_tile_spp, width, height,
                       (width + 7u) / 8u, d_out_film, d_out_half);
    return hipGetLastError();
}

hipError_t launch_length_credit(float* d_length, const uint32_t* d_tile_spp, uint32_t base_spp, float max_history, uint32_t width, uint32_t height,
                                hipStream_t stream) {
    if (adaptive_tile_count(width, height) == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(length_credit_kernel, dim3(pixel_grid(width, height)), dim3(256), 0, stream, d_length, d_tile_spp, base_spp, max_history, width, height,
                       (width + 7u) / 8u);
    return hipGetLastError();
}

}  // namespace pt
