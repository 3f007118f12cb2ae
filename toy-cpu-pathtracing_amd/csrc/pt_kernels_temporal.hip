// The temporal reprojection of include/mi355pt_temporal.h — the temporal half of SVGF (Schied et al., HPG 2017) beside the spatial filter
// of pt_kernels_denoise_var.hip — with its carries (include/mi355pt_motion.h, mi355pt_flow.h) and the gather of its rectified form
// (include/mi355pt_temporal_rectify.h) as one plain HIP kernel template for gfx950.  EXTENSION, no reference counterpart.  It keeps the
// denoisers' shape: one thread per pixel, 64 x 4 blocks, no LDS, no atomics, no scratch.
//
// A pixel's hit position is projected into the previous camera, and the previous frame's accumulated films are gathered with a 2 x 2
// bilinear footprint.  The four taps' loads are UNCONDITIONAL, at indices clamped to the frame: whether a pixel has a history at all (no
// hit, behind the previous camera, outside its image) and whether a tap is valid (in frame, hit, plane distance, normal) are selects on the
// loaded values, never branches around loads — as the 3 x 3 of pt_kernels_denoise_var.hip.  All gathers of a pixel are in flight together.
// Neighbouring lanes reproject to neighbouring texels, so the gathers are served by L1 / L2.  (What the compiler does form is a skip around
// a tap's and the blend's divisions for a wave in which no pixel needs them: arithmetic only, after every load.)
//
// The body stands in the kernel itself, not in functions it calls: with the kernel's arguments reaching it through references the
// compiler groups their loads differently, and schedule, registers and time move.
//
// Every operation is a single binary32 operation in the order the headers state (the unit is built with -ffp-contract=off and calls no
// fmaf), divisions are IEEE: the result is bit-equal to tests/temporal_reference.py, motion_reference.py and flow_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

// CARRY, as TemporalCarryDev::kind: 0 the static world, Xp = X + a.delta.  1 (include/mi355pt_motion.h): the pixel's id picks a record of
// cv.table, which carries X and nrm into the previous render space.  2 (include/mi355pt_flow.h): the pixel's own record of cv.flow is
// ADDED to X and to nrm.  With 1 and 2 a.delta is not read, and with HAS_PREV_IDS a tap must show the pixel's id (cv.ids_cur[p], which the
// records' form does not read otherwise).  HAS_PREV == false: the first frame, which reprojects nothing (prev and cv are not read).
// RECORD == false: the accumulation in one launch, the blend of mi355pt_temporal.h stored into the three outputs (record is not read).
// RECORD == true: the first launch of a rectified form.  No blend, and the current film is not read: the gathered history hist1, hist2
// (hist, 0 without a half film) and L = min(Lh + 1, max_history), or all 0 for a pixel without history, stored as one record per pixel
// (the outputs are not read); the second launch is pt_kernels_temporal_rectify.hip's blend over those records
template <bool HAS_HALF, bool HAS_PREV, int CARRY, bool HAS_PREV_IDS, bool RECORD>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a, TemporalCarryDev cv,
                                                                           float* __restrict__ out_film, float* __restrict__ out_half,
                                                                           float* __restrict__ out_length, float4* __restrict__ record) {
    static_assert(HAS_PREV || (CARRY == 0 && !RECORD), "the first frame reprojects nothing: it is the static, blending form");
    static_assert(CARRY != 0 || !HAS_PREV_IDS, "the static world has no ids");
    const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;

    // the current values (dead with RECORD)
    const float3u B = tp_load3(cur.film, p);
    float c1[3], c2[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (HAS_HALF) {
        const float3u H = tp_load3(cur.half, p);
        c1[0] = dn_clean(H.x, a.half_spp); c1[1] = dn_clean(H.y, a.half_spp); c1[2] = dn_clean(H.z, a.half_spp);
        c2[0] = dn_clean(B.x - H.x, a.half_spp); c2[1] = dn_clean(B.y - H.y, a.half_spp); c2[2] = dn_clean(B.z - H.z, a.half_spp);
    } else {
        c1[0] = dn_clean(B.x, a.spp); c1[1] = dn_clean(B.y, a.spp); c1[2] = dn_clean(B.z, a.spp);
    }
    float m1[3] = {c1[0], c1[1], c1[2]}, m2[3] = {c2[0], c2[1], c2[2]}, L = 1.0f;
    if constexpr (RECORD) {
        m1[0] = m1[1] = m1[2] = 0.0f; m2[0] = m2[1] = m2[2] = 0.0f; L = 0.0f;
    }

    if constexpr (HAS_PREV) {
        // geometry of p (h == 0 makes NaNs and infinities: `ok` selects them away).  The carry's loads are issued ahead of the geometry's
        // divisions: the pixel's own record (two 16-byte loads, coalesced), or its id and then the id's record (six 16-byte loads) — one
        // dependent round trip more than the static world has, and it is over when the quotients are
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
            // a = r0.xyzw r1.xyzw r2.x,  b = r2.yzw,  n = r3.xyzw r4.xyzw r5.x: Xp = a X + b, nrm = n nrm — both in the previous render space
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
        const int wm1 = (int)a.width - 1, hm1 = (int)a.height - 1;

        // the four taps: every load at an index clamped to the frame, issued whatever `ok` and the tap's validity are
        float w[4], len[4], hq[4];
        bool inside[4];
        bool same[4] = {true, true, true, true};          // the tap shows the pixel's instance (always, without the previous frame's ids)
        float3u Pq[4], Nq[4], f[4], g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            inside[k] = qx >= 0 && qx <= wm1 && qy >= 0 && qy <= hm1;
            const int cx = qx < 0 ? 0 : (qx > wm1 ? wm1 : qx), cy = qy < 0 ? 0 : (qy > hm1 ? hm1 : qy);
            const size_t q = (size_t)cy * a.width + (size_t)cx;
            hq[k] = prev.hit[3 * q + 1];
            len[k] = prev.length[q];
            Pq[k] = tp_load3(prev.position, q); Nq[k] = tp_load3(prev.shading_normal, q);
            f[k] = tp_load3(prev.film, q);
            if constexpr (HAS_HALF) g[k] = tp_load3(prev.half, q);
            if constexpr (CARRY != 0 && HAS_PREV_IDS) same[k] = cv.ids_prev[q] == idc;
        }
        // The film values are needed only where the tap turns out valid, and the compiler would sink their loads into a branch on that
        // (it turns a select whose operand is a load into control flow): the gathers would wait for the geometry loads and the arithmetic on
        // them, one tap after the other.  tp_keep pins the loaded values here, after all four taps' loads have been issued
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tp_keep(f[k]);
            if constexpr (HAS_HALF) tp_keep(g[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float ex = Xx - Pq[k].x / hq[k], ey = Xy - Pq[k].y / hq[k], ez = Xz - Pq[k].z / hq[k];
            const float pd = fabsf(tp_dot(ex, ey, ez, nx, ny, nz));
            const float qnx = 2.0f * (Nq[k].x / hq[k]) - 1.0f, qny = 2.0f * (Nq[k].y / hq[k]) - 1.0f, qnz = 2.0f * (Nq[k].z / hq[k]) - 1.0f;
            const float nd = tp_dot(nx, ny, nz, qnx, qny, qnz);
            bool valid = ok && inside[k] && hq[k] > 0.0f && len[k] > 0.0f && pd <= tol && nd >= a.normal_cos;
            if constexpr (CARRY != 0) valid = valid && same[k];
            w[k] = valid ? bw[k] : 0.0f;
            len[k] = valid ? len[k] : 0.0f;
            f[k] = float3u{valid ? f[k].x : 0.0f, valid ? f[k].y : 0.0f, valid ? f[k].z : 0.0f};
            if constexpr (HAS_HALF) g[k] = float3u{valid ? g[k].x : 0.0f, valid ? g[k].y : 0.0f, valid ? g[k].z : 0.0f};
        }
        const float Wt = ((w[0] + w[1]) + w[2]) + w[3];
        const bool has = Wt > a.min_weight;
        const float Lh = (((w[0] * len[0] + w[1] * len[1]) + w[2] * len[2]) + w[3] * len[3]) / Wt;
        const float Lc = fminf(Lh + 1.0f, a.max_history);
        const float alpha = 1.0f / Lc;
        if constexpr (RECORD) L = has ? Lc : 0.0f;
        else L = has ? Lc : 1.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float fv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fv[k] = ch == 0 ? f[k].x : (ch == 1 ? f[k].y : f[k].z);
                if constexpr (HAS_HALF) gv[k] = ch == 0 ? g[k].x : (ch == 1 ? g[k].y : g[k].z);
            }
            if constexpr (HAS_HALF) {
                const float hist1 = (((w[0] * gv[0] + w[1] * gv[1]) + w[2] * gv[2]) + w[3] * gv[3]) / Wt;
                const float hist2 = (((w[0] * (fv[0] - gv[0]) + w[1] * (fv[1] - gv[1])) + w[2] * (fv[2] - gv[2])) + w[3] * (fv[3] - gv[3])) / Wt;
                if constexpr (RECORD) {
                    m1[ch] = has ? hist1 : 0.0f;
                    m2[ch] = has ? hist2 : 0.0f;
                } else {
                    const float b1 = hist1 + (c1[ch] - hist1) * alpha, b2 = hist2 + (c2[ch] - hist2) * alpha;
                    m1[ch] = has ? b1 : c1[ch];
                    m2[ch] = has ? b2 : c2[ch];
                }
            } else {
                const float hist = (((w[0] * fv[0] + w[1] * fv[1]) + w[2] * fv[2]) + w[3] * fv[3]) / Wt;
                if constexpr (RECORD) {
                    m1[ch] = has ? hist : 0.0f;
                } else {
                    const float b1 = hist + (c1[ch] - hist) * alpha;
                    m1[ch] = has ? b1 : c1[ch];
                }
            }
        }
    }

    if constexpr (RECORD) tp_write_record(record, p, m1, m2, L);
    else tp_write_blend<HAS_HALF>(out_film, out_half, out_length, p, m1, m2, L);
}

// the carry's kernel for the frame's films: with or without a half film, with or without the previous frame's ids (a carry's only)
template <bool HAS_PREV, int CARRY, bool RECORD>
void launch_carry(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const TemporalCarryDev& carry, const TemporalOutsDev& outs,
                  float4* record, hipStream_t stream) {
    const TpShape sh = tp_shape(args);
    tp_dispatch(cur.half != nullptr, CARRY != 0 && carry.ids_prev != nullptr, [&](auto half, auto ids) {
        if constexpr (CARRY != 0 || !decltype(ids)::value)
            hipLaunchKernelGGL((temporal_kernel<decltype(half)::value, HAS_PREV, CARRY, decltype(ids)::value, RECORD>), sh.grid, sh.block, 0, stream, cur, prev, args,
                               carry, outs.film, outs.half, outs.length, record);
    });
}

template <bool RECORD>
hipError_t launch_with_prev(const TemporalFrameDev& cur, const TemporalFrameDev& prev, const TemporalArgs& args, const TemporalCarryDev& carry,
                            const TemporalOutsDev& outs, float4* record, hipStream_t stream) {
    switch (carry.kind) {
        case CARRY_STATIC: launch_carry<true, CARRY_STATIC, RECORD>(cur, prev, args, carry, outs, record, stream); break;
        case CARRY_TABLE: launch_carry<true, CARRY_TABLE, RECORD>(cur, prev, args, carry, outs, record, stream); break;
        case CARRY_FLOW: launch_carry<true, CARRY_FLOW, RECORD>(cur, prev, args, carry, outs, record, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_temporal.cpp's driver, which has checked every argument) ----
hipError_t launch_temporal_accumulate(const TemporalFrameDev& cur, const TemporalFrameDev* prev, TemporalArgs args, const TemporalCarryDev& carry,
                                      const TemporalOutsDev& outs, hipStream_t stream) {
    if (prev) return launch_with_prev<false>(cur, *prev, args, carry, outs, nullptr, stream);
    launch_carry<false, CARRY_STATIC, false>(cur, TemporalFrameDev{}, args, TemporalCarryDev{}, outs, nullptr, stream);
    return hipGetLastError();
}

hipError_t launch_temporal_gather(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const TemporalCarryDev& carry, void* d_scratch,
                                  hipStream_t stream) {
    return launch_with_prev<true>(cur, prev, args, carry, TemporalOutsDev{}, (float4*)d_scratch, stream);
}

}  // namespace pt
