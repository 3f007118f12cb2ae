// The motion table of include/mi355pt_motion.h: where the points of each instance were one frame ago, as one affine record per instance
// in the RENDER spaces of the two frames.  Host arithmetic only, no HIP: compiles with a plain C++ compiler
// (tests/motion_plan_check.cpp walks it, also under the host sanitizers); api_motion.cpp's mi355pt_motion_table is this function.
// Everything is computed in double from the f32 inputs; each entry is rounded once to f32.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace pt {

// mi355pt_motion_xform, field for field (api_motion.cpp asserts the sizes agree)
struct MotionXform { float a[9], b[3], n[9], pad[3]; };

// The linear part of a column-major 4x4 as a ROW-major 3x3 in double and its inverse (row-major).  false: the matrix has a non-finite
// entry, the determinant of its linear part is exactly zero, or the inverse is not finite — what the lowering refuses (scene_lower.cpp
// lower_transform, instance_transform_ok)
inline bool motion_linear_inverse(const float* m4, double lin[9], double inv[9]) {
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m4[k])) return false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) lin[3 * r + c] = (double)m4[4 * c + r];
    const double* a = lin;
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double adj[9] = {c00, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           c01, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           c02, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    for (int k = 0; k < 9; ++k) {
        inv[k] = adj[k] / det;
        if (!std::isfinite(inv[k])) return false;
    }
    return true;
}

inline void motion_mul3(const double x[9], const double y[9], double o[9]) {   // o = x y, row-major
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[3 * r + c] = (x[3 * r] * y[c] + x[3 * r + 1] * y[3 + c]) + x[3 * r + 2] * y[6 + c];
}

// the static record: a = n = I, b = c_cur - c_prev (mi355pt_temporal_view::delta, the same expression: the same bits)
inline void motion_static_entry(const float c_cur[3], const float c_prev[3], MotionXform* out) {
    std::memset(out, 0, sizeof(*out));
    out->a[0] = out->a[4] = out->a[8] = 1.0f;
    out->n[0] = out->n[4] = out->n[8] = 1.0f;
    for (int i = 0; i < 3; ++i) out->b[i] = (float)((double)c_cur[i] - (double)c_prev[i]);
}

// out[0 .. n]: record 0 static, record i + 1 of instance i.  l2w_cur / l2w_prev: n column-major 4x4 each.  false (nothing written): n == 0
// or a matrix motion_linear_inverse refuses — of a moved and of an unmoved instance alike
inline bool motion_table(const float c_cur[3], const float c_prev[3], const float* l2w_cur, const float* l2w_prev, uint32_t n, MotionXform* out) {
    if (n == 0u) return false;
    double lin[9], inv[9];
    for (uint32_t i = 0; i < n; ++i)
        if (!motion_linear_inverse(l2w_cur + 16 * (size_t)i, lin, inv) || !motion_linear_inverse(l2w_prev + 16 * (size_t)i, lin, inv)) return false;
    motion_static_entry(c_cur, c_prev, &out[0]);
    for (uint32_t i = 0; i < n; ++i) {
        const float *mc = l2w_cur + 16 * (size_t)i, *mp = l2w_prev + 16 * (size_t)i;
        MotionXform* e = &out[(size_t)i + 1];
        motion_static_entry(c_cur, c_prev, e);
        if (std::memcmp(mc, mp, 16 * sizeof(float)) == 0) continue;                 // did not move: the static record exactly
        double ac[9], aci[9], ap[9], api[9], a[9], ai[9];
        motion_linear_inverse(mc, ac, aci);
        motion_linear_inverse(mp, ap, api);
        motion_mul3(ap, aci, a);                                                    // lin(T) = A_prev A_cur^-1
        motion_mul3(ac, api, ai);                                                   // its inverse = A_cur A_prev^-1
        for (int r = 0; r < 3; ++r) {
            // trans(T) = t_prev - a t_cur;  b = a c_cur + trans(T) - c_prev = a (c_cur - t_cur) + (t_prev - c_prev)
            double s = 0.0;
            for (int c = 0; c < 3; ++c) s += a[3 * r + c] * ((double)c_cur[c] - (double)mc[12 + c]);
            e->b[r] = (float)(s + ((double)mp[12 + r] - (double)c_prev[r]));
            for (int c = 0; c < 3; ++c) {
                e->a[3 * r + c] = (float)a[3 * r + c];
                e->n[3 * r + c] = (float)ai[3 * c + r];                             // (a^-1)^T
            }
        }
    }
    return true;
}

}  // namespace pt
