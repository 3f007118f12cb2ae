// Moving instances of a built scene (include/mi355pt_instances.h): the arithmetic host and device share.  Pure — no HIP header, no
// environment, no clock — like rebase_plan.hpp; tests/instance_move_plan_check.cpp includes it alone.  Three things live here:
//
//   1. THE geometric normal of a shading record (DevTriShade::ng): normalize(normalize(cross(p1 - p0, p2 - p0))) of the LOCAL vertices,
//      carried through the instance's inverse-transpose, renormalised.  scene_lower.cpp lower_triangles and shade_refresh_kernel
//      (pt_kernels_instances.hip) both call shade_normal below; every step is one binary32 operation (the units are compiled without
//      contraction), the division and the square root are correctly rounded on both sides.
//   2. An emissive triangle's light_pdf_area from the area tables, the one expression lower_triangles and lower_camera_records use.
//   3. The SAH cost of a refit BVH2: one term per used (node, side) of the refit plan's entries, summed in ONE fixed order — blocks of
//      SAH_BLOCK terms in a stride-halving tree, then the block sums the same way, level by level, until one is left — and divided by the
//      half area of the root.  sah_terms_kernel / sah_finish_kernel walk exactly this order with one thread per tree lane; sah_cost_host
//      walks it in a loop.  No term order depends on scheduling, so the two values are bit-equal.
#pragma once
#include <cstdint>
#include <vector>

#include "layout.hpp"
#include "rebase_plan.hpp"

namespace pt {

// ---- 1. the geometric normal ----
struct IV3 { float x, y, z; };
PT_HD inline IV3 iv_sub(IV3 a, IV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
PT_HD inline IV3 iv_cross(IV3 a, IV3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
PT_HD inline float iv_dot(IV3 a, IV3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
PT_HD inline float iv_length(IV3 a) { return __builtin_sqrtf(iv_dot(a, a)); }
PT_HD inline IV3 iv_normalize(IV3 a) { const float r = 1.0f / iv_length(a); return {a.x * r, a.y * r, a.z * r}; }

// inv: DevInstance::inv (its first 9 floats: the linear part of render_to_local, column-major); identity: DevInstance::identity
PT_HD inline IV3 shade_normal(IV3 p0, IV3 p1, IV3 p2, const float* inv, bool identity) {
    IV3 n = iv_normalize(iv_normalize(iv_cross(iv_sub(p1, p0), iv_sub(p2, p0))));
    if (!identity)
        n = IV3{(inv[0] * n.x + inv[1] * n.y) + inv[2] * n.z, (inv[3] * n.x + inv[4] * n.y) + inv[5] * n.z, (inv[6] * n.x + inv[7] * n.y) + inv[8] * n.z};
    return iv_normalize(n);
}

// ---- 2. light_pdf_area of triangle t of an area light (emissive_triangle_mesh.rs:334-353) ----
inline float light_pdf_area_of(const std::vector<float>& area, const std::vector<float>& cdf, uint32_t t) {
    const float probability = t == 0 ? cdf[0] : cdf[t] - cdf[t - 1];
    return 1.0f / area[t] * probability;
}

// ---- 3. the SAH cost ----
constexpr uint32_t SAH_BLOCK = 256;

PT_HD inline float half_area(const float lo[3], const float hi[3]) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return (dx * dy + dy * dz) + dz * dx;
}
// the term of entry (node, side): half area of the child box x (1 for an inner child, the triangle count for a leaf)
PT_HD inline float sah_term(const DevNode& n, int side) {
    const float lo[3] = {n.bx[side], n.by[side], n.bz[side]}, hi[3] = {n.bx[2 + side], n.by[2 + side], n.bz[2 + side]};
    const int32_t link = n.child[side];
    return half_area(lo, hi) * (link < 0 ? (float)leaf_count(link) : 1.0f);
}
// a(root): the half area of the union of the root record's used child boxes
PT_HD inline float root_half_area(const DevNode& root) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool any = false;
    for (int side = 0; side < 2; ++side) {
        if (!child_used(root, side)) continue;
        any = true;
        lo[0] = rb_min(lo[0], root.bx[side]); lo[1] = rb_min(lo[1], root.by[side]); lo[2] = rb_min(lo[2], root.bz[side]);
        hi[0] = rb_max(hi[0], root.bx[2 + side]); hi[1] = rb_max(hi[1], root.by[2 + side]); hi[2] = rb_max(hi[2], root.bz[2 + side]);
    }
    return any ? half_area(lo, hi) : 0.0f;
}
// sum / a(root); a root without area (no node, or boxes without extent) has cost 0 / 0, reported as 0
PT_HD inline float sah_quotient(float sum, float area) { return area > 0.0f ? sum / area : 0.0f; }

// one lane's step of the stride-halving tree over v[0 .. SAH_BLOCK): lane t < s adds the value s places up.  The device runs the lanes
// of a stride side by side between two barriers, the host one after the other: the operands of every addition are the same.
PT_HD inline void sah_tree_step(float* v, uint32_t t, uint32_t s) { v[t] = v[t] + v[t + s]; }
inline uint32_t sah_blocks(uint32_t n) { return (n + SAH_BLOCK - 1u) / SAH_BLOCK; }

// the sum of one block of up to SAH_BLOCK values (missing ones count as +0.0), on the host
inline float sah_block_sum_host(const float* values, uint32_t count) {
    float v[SAH_BLOCK];
    for (uint32_t t = 0; t < SAH_BLOCK; ++t) v[t] = t < count ? values[t] : 0.0f;
    for (uint32_t s = SAH_BLOCK / 2; s > 0; s >>= 1) for (uint32_t t = 0; t < s; ++t) sah_tree_step(v, t, s);
    return v[0];
}
// the fixed-order sum of n terms: block sums, then block sums of those, until one value is left (0 terms: 0)
inline float sah_sum_host(std::vector<float> terms) {
    if (terms.empty()) return 0.0f;
    bool first = true;                                                // (a single term still goes through one block: + 0.0 255 times)
    while (first || terms.size() > 1) {
        first = false;
        const uint32_t n = (uint32_t)terms.size(), nb = sah_blocks(n);
        for (uint32_t b = 0; b < nb; ++b) terms[b] = sah_block_sum_host(terms.data() + (size_t)b * SAH_BLOCK, n - b * SAH_BLOCK < SAH_BLOCK ? n - b * SAH_BLOCK : SAH_BLOCK);
        terms.resize(nb);
    }
    return terms[0];
}
// the SAH cost of the BVH2 `nodes` over the plan's entries (all height groups, in the plan's order)
inline float sah_cost_host(const std::vector<DevNode>& nodes, int32_t root, const std::vector<uint32_t>& entries) {
    if (root < 0 || nodes.empty() || entries.empty()) return 0.0f;
    std::vector<float> terms(entries.size());
    for (size_t k = 0; k < entries.size(); ++k) terms[k] = sah_term(nodes[entries[k] >> 1], (int)(entries[k] & 1u));
    return sah_quotient(sah_sum_host(std::move(terms)), root_half_area(nodes[(size_t)root]));
}

}  // namespace pt
