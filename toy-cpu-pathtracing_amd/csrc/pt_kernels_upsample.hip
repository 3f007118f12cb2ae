// The guided half-resolution upsample of include/mi355pt_upsample.h — a joint-bilateral upsample (Kopf et al., SIGGRAPH 2007) of a film traced
// at W/2 x H/2, guided by the G-buffers of both resolutions — as one HIP kernel for gfx950.  EXTENSION, no reference counterpart.  It keeps
// the filters' shape: one thread per FULL pixel, 64 x 4 blocks, no atomics, no scratch.
//
// Two forms of the same arithmetic, bit-equal to each other:
//   upsample_kernel          the DIRECT GATHER, built first: a full pixel reads its own guide values and the 2 x 2 low taps around it from
//                            global memory.  The taps' loads are UNCONDITIONAL, at indices clamped to the low frame: whether a tap is valid (in
//                            frame, same surface: plane distance, normal, emitter share; background to background) is a select on the loaded
//                            values, never a branch around loads — as pt_kernels_temporal.hip, whose helpers (pt_temporal_gather.hpp) this unit takes.  A low tap is read
//                            by up to 16 full pixels, and each of them repeats the tap's divisions.
//   upsample_staged_kernel   the block's 34 x 4 low pixels and what is derived from them, once, in LDS.  tools/upsample_rate.py found the direct
//                            gather at 1.9 - 2.7 times a copy of its compulsory bytes, the staged form at 1.25 - 1.43 times and 0.54 - 0.68 of
//                            the direct gather's time (profiles/upsample_rate.json): the launcher takes this one.
// The parent tap (x >> 1, y >> 1) is always one of the four and always in the frame, so the fallback costs no load of its own.
//
// Every operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls no
// fmaf), divisions are IEEE: the result is bit-equal to tests/upsample_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

__device__ __forceinline__ float up_pick(const float3u& v, int ch) { return ch == 0 ? v.x : (ch == 1 ? v.y : v.z); }
// channel ch of the parent tap kp: the fallback's value (selects on register values: an index into the array would put it in scratch)
__device__ __forceinline__ float up_parent(const float3u (&c)[4], int kp, int ch) {
    const float v0 = up_pick(c[0], ch), v1 = up_pick(c[1], ch), v2 = up_pick(c[2], ch), v3 = up_pick(c[3], ch);
    const float lo = (kp & 1) ? v1 : v0, hi = (kp & 1) ? v3 : v2;
    return (kp & 2) ? hi : lo;
}

template <bool HAS_HALF, bool HAS_ALBEDO>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void upsample_kernel(const float* __restrict__ low_film, const float* __restrict__ low_half,
                                                                           UpsampleGuidesDev lg, UpsampleGuidesDev fg, UpsampleArgs a,
                                                                           float* __restrict__ out_film, float* __restrict__ out_half) {
    const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const uint32_t lw = a.width >> 1, lh = a.height >> 1;      // the low frame (width and height are even: x >> 1 < lw, y >> 1 < lh)

    // the full pixel's geometry (hp == 0 makes NaNs and infinities: `surface` selects them away)
    const float3u P = tp_load3(fg.position, p), N = tp_load3(fg.shading_normal, p), Hp = tp_load3(fg.hit, p);
    float3u Ap{0.0f, 0.0f, 0.0f};
    if constexpr (HAS_ALBEDO) Ap = tp_load3(fg.albedo, p);
    const float hp = Hp.y;
    const bool surface = hp > 0.0f;
    const float Xx = P.x / hp, Xy = P.y / hp, Xz = P.z / hp;
    const float nx = 2.0f * (N.x / hp) - 1.0f, ny = 2.0f * (N.y / hp) - 1.0f, nz = 2.0f * (N.z / hp) - 1.0f;
    const float t = Hp.x / hp, em = Hp.z / hp;
    const float tol = a.pos_tol * t;

    // the footprint: an even x sits left of its parent's centre (taps X - 1 and X, the parent with 0.75), an odd x right of it
    const bool xe = (x & 1u) == 0u, ye = (y & 1u) == 0u;
    const int x0 = (int)(x >> 1) - (xe ? 1 : 0), y0 = (int)(y >> 1) - (ye ? 1 : 0);
    const float wx = xe ? 0.75f : 0.25f, wy = ye ? 0.75f : 0.25f;
    const float omx = 1.0f - wx, omy = 1.0f - wy;
    const float bw[4] = {omx * omy, wx * omy, omx * wy, wx * wy};
    const int kp = (xe ? 1 : 0) | (ye ? 2 : 0);                // the parent's tap
    const int wm1 = (int)lw - 1, hm1 = (int)lh - 1;

    // the four taps: every load at an index clamped to the low frame, issued whatever the tap's validity is
    bool inside[4];
    float3u Hq[4], Pq[4], Nq[4], Aq[4], f[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        inside[k] = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
        const int cx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
        const size_t q = (size_t)cy * lw + (size_t)cx;
        Hq[k] = tp_load3(lg.hit, q);
        Pq[k] = tp_load3(lg.position, q); Nq[k] = tp_load3(lg.shading_normal, q);
        if constexpr (HAS_ALBEDO) Aq[k] = tp_load3(lg.albedo, q);
        f[k] = tp_load3(low_film, q);
        if constexpr (HAS_HALF) g[k] = tp_load3(low_half, q);
    }
    // the compiler would sink the loads of values that only a valid tap needs into a branch on its validity (pt_kernels_temporal.hip):
    // tp_keep pins them here, after all four taps' loads have been issued
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tp_keep(f[k]);
        if constexpr (HAS_HALF) tp_keep(g[k]);
        if constexpr (HAS_ALBEDO) tp_keep(Aq[k]);
    }

    float w[4];
    float3u c1[4], c2[4], i1[4], i2[4];       // the cleaned tap values and what enters the sums (c, i and 0 without a half film)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (HAS_HALF) {
            c1[k] = float3u{dn_clean(g[k].x, a.half_spp), dn_clean(g[k].y, a.half_spp), dn_clean(g[k].z, a.half_spp)};
            c2[k] = float3u{dn_clean(f[k].x - g[k].x, a.half_spp), dn_clean(f[k].y - g[k].y, a.half_spp), dn_clean(f[k].z - g[k].z, a.half_spp)};
        } else {
            c1[k] = float3u{dn_clean(f[k].x, a.spp), dn_clean(f[k].y, a.spp), dn_clean(f[k].z, a.spp)};
            c2[k] = float3u{0.0f, 0.0f, 0.0f};
        }
        const float hq = Hq[k].y;
        const float ex = Xx - Pq[k].x / hq, ey = Xy - Pq[k].y / hq, ez = Xz - Pq[k].z / hq;
        const float pd = fabsf(tp_dot(ex, ey, ez, nx, ny, nz));
        const float qnx = 2.0f * (Nq[k].x / hq) - 1.0f, qny = 2.0f * (Nq[k].y / hq) - 1.0f, qnz = 2.0f * (Nq[k].z / hq) - 1.0f;
        const float nd = tp_dot(nx, ny, nz, qnx, qny, qnz);
        const float ed = fabsf(em - Hq[k].z / hq);
        const bool same = hq > 0.0f && pd <= tol && nd >= a.normal_cos && ed <= a.emitter_tol;
        const bool valid = inside[k] && (surface ? same : hq == 0.0f);
        w[k] = valid ? bw[k] : 0.0f;
        float3u v1 = c1[k], v2 = c2[k];
        if constexpr (HAS_ALBEDO) {
            const float dx = dn_clip0(Aq[k].x, a.spp_albedo_low) + a.albedo_eps, dy = dn_clip0(Aq[k].y, a.spp_albedo_low) + a.albedo_eps,
                        dz = dn_clip0(Aq[k].z, a.spp_albedo_low) + a.albedo_eps;
            v1 = float3u{surface ? c1[k].x / dx : c1[k].x, surface ? c1[k].y / dy : c1[k].y, surface ? c1[k].z / dz : c1[k].z};
            if constexpr (HAS_HALF) v2 = float3u{surface ? c2[k].x / dx : c2[k].x, surface ? c2[k].y / dy : c2[k].y, surface ? c2[k].z / dz : c2[k].z};
        }
        i1[k] = float3u{valid ? v1.x : 0.0f, valid ? v1.y : 0.0f, valid ? v1.z : 0.0f};
        i2[k] = float3u{valid ? v2.x : 0.0f, valid ? v2.y : 0.0f, valid ? v2.z : 0.0f};
    }
    const float Wt = ((w[0] + w[1]) + w[2]) + w[3];
    const bool has = Wt > a.min_weight;

    float m1[3], m2[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float re = 1.0f;                      // a_p + albedo_eps: what the interpolated value is multiplied by
        if constexpr (HAS_ALBEDO) re = dn_clip0(up_pick(Ap, ch), a.spp_albedo_full) + a.albedo_eps;
        {
            const float s = ((w[0] * up_pick(i1[0], ch) + w[1] * up_pick(i1[1], ch)) + w[2] * up_pick(i1[2], ch)) + w[3] * up_pick(i1[3], ch);
            float i = s / Wt;
            if constexpr (HAS_ALBEDO) i = surface ? i * re : i;
            m1[ch] = has ? i : up_parent(c1, kp, ch);
        }
        if constexpr (HAS_HALF) {
            const float s = ((w[0] * up_pick(i2[0], ch) + w[1] * up_pick(i2[1], ch)) + w[2] * up_pick(i2[2], ch)) + w[3] * up_pick(i2[3], ch);
            float i = s / Wt;
            if constexpr (HAS_ALBEDO) i = surface ? i * re : i;
            m2[ch] = has ? i : up_parent(c2, kp, ch);
        }
    }

    if constexpr (HAS_HALF) {
        out_half[3 * p] = m1[0]; out_half[3 * p + 1] = m1[1]; out_half[3 * p + 2] = m1[2];
        out_film[3 * p] = m1[0] + m2[0]; out_film[3 * p + 1] = m1[1] + m2[1]; out_film[3 * p + 2] = m1[2] + m2[2];
    } else {
        out_film[3 * p] = m1[0]; out_film[3 * p + 1] = m1[1]; out_film[3 * p + 2] = m1[2];
    }
}

// ---- the LDS-staged form ----
// The direct gather above does a tap's arithmetic — its normalised position, normal and emitter share, its cleaned and demodulated film
// values: up to 22 IEEE divisions — once per full pixel that reads the tap, up to 16 times.  A 64 x 4 block of full pixels reads 34 x 4 low
// pixels (32 x 2 parents and a ring of one).  This form has the block's first 136 threads load one low pixel each (at an index clamped to the
// low frame, as above), do that arithmetic ONCE and store the results as planes of 136 words in LDS; after the barrier a full pixel reads
// its four taps from there.  The operations and their operands are those of the direct gather, so the result is the same bits.
constexpr int UP_TILE_W = DN_BLOCK_X / 2 + 2, UP_TILE_H = DN_BLOCK_Y / 2 + 2, UP_TILE = UP_TILE_W * UP_TILE_H;
// planes: hq; position / hq (3); 2 (normal / hq) - 1 (3); hit.z / hq; c1 (3); c2 (3, with a half film); c1 / (a_q + eps), c2 / (a_q + eps) (with albedo)
constexpr int UP_HQ = 0, UP_P = 1, UP_N = 4, UP_EM = 7, UP_C1 = 8;
template <bool HAS_HALF, bool HAS_ALBEDO>
struct UpPlanes {
    static constexpr int C2 = UP_C1 + 3, D1 = UP_C1 + (HAS_HALF ? 6 : 3), D2 = D1 + 3, COUNT = D1 + (HAS_ALBEDO ? (HAS_HALF ? 6 : 3) : 0);
};

template <bool HAS_HALF, bool HAS_ALBEDO>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void upsample_staged_kernel(const float* __restrict__ low_film, const float* __restrict__ low_half,
                                                                                  UpsampleGuidesDev lg, UpsampleGuidesDev fg, UpsampleArgs a,
                                                                                  float* __restrict__ out_film, float* __restrict__ out_half) {
    using PL = UpPlanes<HAS_HALF, HAS_ALBEDO>;
    __shared__ float s[PL::COUNT * UP_TILE];
    const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    const bool in_frame = x < a.width && y < a.height;
    const size_t p = (size_t)y * a.width + x;
    const uint32_t lw = a.width >> 1, lh = a.height >> 1;
    const int wm1 = (int)lw - 1, hm1 = (int)lh - 1;
    const int tile_x0 = (int)(bx * (DN_BLOCK_X / 2)) - 1, tile_y0 = (int)(by * (DN_BLOCK_Y / 2)) - 1;      // the tile's first low pixel

    // the full pixel's own loads first: they are in flight while the tile is built
    float3u P{0.0f, 0.0f, 0.0f}, N{0.0f, 0.0f, 0.0f}, Hp{0.0f, 0.0f, 0.0f}, Ap{0.0f, 0.0f, 0.0f};
    if (in_frame) {
        P = tp_load3(fg.position, p); N = tp_load3(fg.shading_normal, p); Hp = tp_load3(fg.hit, p);
        if constexpr (HAS_ALBEDO) Ap = tp_load3(fg.albedo, p);
    }

    const int tid = (int)(threadIdx.y * DN_BLOCK_X + threadIdx.x);
    if (tid < UP_TILE) {
        const int qx = tile_x0 + tid % UP_TILE_W, qy = tile_y0 + tid / UP_TILE_W;
        const int cx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
        const size_t q = (size_t)cy * lw + (size_t)cx;
        const float3u Hq = tp_load3(lg.hit, q), Pq = tp_load3(lg.position, q), Nq = tp_load3(lg.shading_normal, q), f = tp_load3(low_film, q);
        float3u g{0.0f, 0.0f, 0.0f}, Aq{0.0f, 0.0f, 0.0f};
        if constexpr (HAS_HALF) g = tp_load3(low_half, q);
        if constexpr (HAS_ALBEDO) Aq = tp_load3(lg.albedo, q);
        const float hq = Hq.y;
        float* o = s + tid;
        o[UP_HQ * UP_TILE] = hq;
        o[(UP_P + 0) * UP_TILE] = Pq.x / hq; o[(UP_P + 1) * UP_TILE] = Pq.y / hq; o[(UP_P + 2) * UP_TILE] = Pq.z / hq;
        o[(UP_N + 0) * UP_TILE] = 2.0f * (Nq.x / hq) - 1.0f; o[(UP_N + 1) * UP_TILE] = 2.0f * (Nq.y / hq) - 1.0f; o[(UP_N + 2) * UP_TILE] = 2.0f * (Nq.z / hq) - 1.0f;
        o[UP_EM * UP_TILE] = Hq.z / hq;
        float c1[3], c2[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (HAS_HALF) {
            c1[0] = dn_clean(g.x, a.half_spp); c1[1] = dn_clean(g.y, a.half_spp); c1[2] = dn_clean(g.z, a.half_spp);
            c2[0] = dn_clean(f.x - g.x, a.half_spp); c2[1] = dn_clean(f.y - g.y, a.half_spp); c2[2] = dn_clean(f.z - g.z, a.half_spp);
        } else {
            c1[0] = dn_clean(f.x, a.spp); c1[1] = dn_clean(f.y, a.spp); c1[2] = dn_clean(f.z, a.spp);
        }
        float den[3] = {1.0f, 1.0f, 1.0f};
        if constexpr (HAS_ALBEDO) {
            den[0] = dn_clip0(Aq.x, a.spp_albedo_low) + a.albedo_eps; den[1] = dn_clip0(Aq.y, a.spp_albedo_low) + a.albedo_eps;
            den[2] = dn_clip0(Aq.z, a.spp_albedo_low) + a.albedo_eps;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            o[(UP_C1 + ch) * UP_TILE] = c1[ch];
            if constexpr (HAS_HALF) o[(PL::C2 + ch) * UP_TILE] = c2[ch];
            if constexpr (HAS_ALBEDO) {
                o[(PL::D1 + ch) * UP_TILE] = c1[ch] / den[ch];
                if constexpr (HAS_HALF) o[(PL::D2 + ch) * UP_TILE] = c2[ch] / den[ch];
            }
        }
    }
    __syncthreads();
    if (!in_frame) return;

    const float hp = Hp.y;
    const bool surface = hp > 0.0f;
    const float Xx = P.x / hp, Xy = P.y / hp, Xz = P.z / hp;
    const float nx = 2.0f * (N.x / hp) - 1.0f, ny = 2.0f * (N.y / hp) - 1.0f, nz = 2.0f * (N.z / hp) - 1.0f;
    const float t = Hp.x / hp, em = Hp.z / hp;
    const float tol = a.pos_tol * t;
    const bool xe = (x & 1u) == 0u, ye = (y & 1u) == 0u;
    const int x0 = (int)(x >> 1) - (xe ? 1 : 0), y0 = (int)(y >> 1) - (ye ? 1 : 0);
    const float wx = xe ? 0.75f : 0.25f, wy = ye ? 0.75f : 0.25f;
    const float omx = 1.0f - wx, omy = 1.0f - wy;
    const float bw[4] = {omx * omy, wx * omy, omx * wy, wx * wy};
    const int t0 = (y0 - tile_y0) * UP_TILE_W + (x0 - tile_x0);          // the tile index of tap 0: 0 .. UP_TILE - UP_TILE_W - 2
    const int tpar = t0 + (xe ? 1 : 0) + (ye ? UP_TILE_W : 0);          // ... and of the parent
    // a surface pixel with albedo takes the demodulated planes, every other pixel the cleaned ones
    const int v1 = (HAS_ALBEDO && surface ? PL::D1 : UP_C1) * UP_TILE, v2 = (HAS_ALBEDO && surface ? PL::D2 : PL::C2) * UP_TILE;

    float w[4], i1[4][3], i2[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const bool inside = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
        const float* r = s + t0 + (k & 1) + (k >> 1) * UP_TILE_W;
        const float hq = r[UP_HQ * UP_TILE];
        const float ex = Xx - r[(UP_P + 0) * UP_TILE], ey = Xy - r[(UP_P + 1) * UP_TILE], ez = Xz - r[(UP_P + 2) * UP_TILE];
        const float pd = fabsf(tp_dot(ex, ey, ez, nx, ny, nz));
        const float nd = tp_dot(nx, ny, nz, r[(UP_N + 0) * UP_TILE], r[(UP_N + 1) * UP_TILE], r[(UP_N + 2) * UP_TILE]);
        const float ed = fabsf(em - r[UP_EM * UP_TILE]);
        const bool same = hq > 0.0f && pd <= tol && nd >= a.normal_cos && ed <= a.emitter_tol;
        const bool valid = inside && (surface ? same : hq == 0.0f);
        w[k] = valid ? bw[k] : 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float u1 = r[v1 + ch * UP_TILE];
            i1[k][ch] = valid ? u1 : 0.0f;
            if constexpr (HAS_HALF) {
                const float u2 = r[v2 + ch * UP_TILE];
                i2[k][ch] = valid ? u2 : 0.0f;
            }
        }
    }
    const float Wt = ((w[0] + w[1]) + w[2]) + w[3];
    const bool has = Wt > a.min_weight;
    float m1[3], m2[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float re = 1.0f;
        if constexpr (HAS_ALBEDO) re = dn_clip0(up_pick(Ap, ch), a.spp_albedo_full) + a.albedo_eps;
        {
            const float sum = ((w[0] * i1[0][ch] + w[1] * i1[1][ch]) + w[2] * i1[2][ch]) + w[3] * i1[3][ch];
            float i = sum / Wt;
            if constexpr (HAS_ALBEDO) i = surface ? i * re : i;
            m1[ch] = has ? i : s[(UP_C1 + ch) * UP_TILE + tpar];
        }
        if constexpr (HAS_HALF) {
            const float sum = ((w[0] * i2[0][ch] + w[1] * i2[1][ch]) + w[2] * i2[2][ch]) + w[3] * i2[3][ch];
            float i = sum / Wt;
            if constexpr (HAS_ALBEDO) i = surface ? i * re : i;
            m2[ch] = has ? i : s[(PL::C2 + ch) * UP_TILE + tpar];
        }
    }
    if constexpr (HAS_HALF) {
        out_half[3 * p] = m1[0]; out_half[3 * p + 1] = m1[1]; out_half[3 * p + 2] = m1[2];
        out_film[3 * p] = m1[0] + m2[0]; out_film[3 * p + 1] = m1[1] + m2[1]; out_film[3 * p + 2] = m1[2] + m2[2];
    } else {
        out_film[3 * p] = m1[0]; out_film[3 * p + 1] = m1[1]; out_film[3 * p + 2] = m1[2];
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_upsample.cpp, which has checked every argument) ----
hipError_t launch_upsample(const float* d_low_film, const float* d_low_half, const UpsampleGuidesDev& low, const UpsampleGuidesDev& full, UpsampleArgs args,
                           float* d_out_film, float* d_out_half, hipStream_t stream) {
    args.blocks_x = (uint32_t)(((uint64_t)args.width + DN_BLOCK_X - 1) / DN_BLOCK_X);
    const dim3 grid(denoise_grid_blocks(args.width, args.height)), block(DN_BLOCK_X, DN_BLOCK_Y);
    const bool has_half = d_low_half != nullptr, has_albedo = full.albedo != nullptr;
    // which form runs: tools/upsample_rate.py measured both (profiles/upsample_rate.json; -DPT_UPSAMPLE_DIRECT builds the other for such a run)
#ifdef PT_UPSAMPLE_DIRECT
#define PT_UP_KERNEL upsample_kernel
#else
#define PT_UP_KERNEL upsample_staged_kernel
#endif
#define PT_UP_LAUNCH(HALF, ALBEDO) \
    hipLaunchKernelGGL((PT_UP_KERNEL<HALF, ALBEDO>), grid, block, 0, stream, d_low_film, d_low_half, low, full, args, d_out_film, d_out_half)
    if (has_half && has_albedo) PT_UP_LAUNCH(true, true);
    else if (has_half) PT_UP_LAUNCH(true, false);
    else if (has_albedo) PT_UP_LAUNCH(false, true);
    else PT_UP_LAUNCH(false, false);
#undef PT_UP_LAUNCH
#undef PT_UP_KERNEL
    return hipGetLastError();
}

}  // namespace pt
