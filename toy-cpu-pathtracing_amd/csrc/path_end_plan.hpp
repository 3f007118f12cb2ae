// EARLY PATH END (pt_kernel_body.inc, the kernels with one tail queue): whether a path survives the NEXT vertex's Russian roulette and depth
// test does not depend on what its next ray hits — the throughput update T *= f / pdf, the draw and the depth are all known when the tail of
// the vertex has sampled the BSDF.  A path that will end there whatever the ray hits is DOOMED: its ray can still change L only by finding an
// emitter (or, the reference's NaN rule, through a non-finite throughput or MIS weight).  The pass that runs the tail therefore takes the
// roulette decision itself, draw included, and ends a doomed path at once when its ray cannot matter.  This header is that decision as pure
// functions, host and device (no HIP in it: tests/path_end_check.cpp runs them on the CPU against restatements of the front's statements and
// of the traversals' triangle test); the kernel calls these and nothing else for it.
//   1. path_end_pmax / path_end_draws / path_end_doomed: the front's roulette and depth test (pt_path.hpp shade_vertex_head), same expressions
//      in the same order (-ffp-contract=off), on the values the pass holds.
//   2. path_end_term_is_zero: the term the front adds to L at a hit that is no emitter, (T * 0) * w.
//   3. light_box_may_reach: a ray against an area light's padded render-space box; light_boxes(): those boxes on the host.
#pragma once
#include <cstdint>
#include <vector>

#include "layout.hpp"

namespace pt {

// the flag a doomed path carries from the pass to its next front, where it replaces the draw: Path::depth's top bit (max_depth <= 1000)
constexpr uint32_t PATH_DOOMED_BIT = 0x80000000u;

PT_HD inline float pe_max(float a, float b) { return a < b ? b : a; }          // (no NaN reaches these: see the callers)
PT_HD inline float pe_min(float a, float b) { return b < a ? b : a; }
PT_HD inline float pe_abs(float v) { return v < 0.0f ? -v : v; }
// fmaxf's rule: a NaN operand is ignored (the front folds max(T) with fmaxf from -inf)
PT_HD inline float pe_fmax(float a, float b) { return (b != b) ? a : ((a != a) ? b : (a < b ? b : a)); }

// ---- 1. the roulette and the depth test of the next front ----
// max over the wavelengths of the throughput the next front will hold: T[i] * (pf[i] * (1 / p_pdf)), apply_russian_roulette's p
PT_HD inline float path_end_pmax(const float T[4], const float pf[4], float p_pdf) {
    const float tf = 1.0f / p_pdf;
    float p = -__builtin_huge_valf();
    for (int i = 0; i < 4; ++i) p = pe_fmax(p, T[i] * (pf[i] * tf));
    return p;
}
// does the roulette draw a number at that vertex?  (a NaN p draws, like the front: !(p >= gate))
PT_HD inline bool path_end_draws(float p, float rr_gate) { return !(p >= rr_gate); }
// does the path end at that vertex whatever its ray hits?  `ur`: the draw, read only when path_end_draws(p, rr_gate).  `depth`: the path's
// depth now (the front would add one and compare)
PT_HD inline bool path_end_doomed(float p, float ur, float rr_gate, uint32_t depth, uint32_t max_depth) {
    if (path_end_draws(p, rr_gate) && !(ur < p)) return true;
    return depth + 1u > max_depth;
}

// ---- 2. the term of a hit that is no emitter ----
// The front adds (T[i] * 0.0f) * w to L there: +-0, unless T or w is inf or NaN — then NaN, which the sample keeps like the reference's.
// Only a term that compares equal to zero in all four wavelengths may go unadded (L never holds -0: it starts at +0 and only sums).
PT_HD inline bool path_end_term_is_zero(const float T[4], float w) {
    bool zero = true;
    for (int i = 0; i < 4; ++i) zero = zero && ((T[i] * 0.0f) * w == 0.0f);
    return zero;
}

// ---- 3. can the ray reach an area light? ----
// A box record: lo.xyz, the host's pad, hi.xyz, 0 — 32 bytes, stored UNPADDED; an empty box (lo > hi: a light that is no area light)
// is reached by nothing.
constexpr uint32_t LIGHT_BOX_FLOATS = 8u;
// THE PAD.  A skipped ray must be one that none of the traversals' triangle tests (pt_device.hpp intersect_triangle: watertight, on
// vertices translated by the ray origin in f32) would report on a triangle inside the box.  What separates that test from the exact geometry:
// the rounding of v - o (half an ulp of |v| + |o| per axis), of the local-space form's o + tri_shift and of its vertices (render - shift
// rounded once more: half an ulp of the render coordinate plus the shift), and the edge functions' relative error, a few ulp of the same
// lengths; the slab test below adds one rounding per subtraction and product, again relative to |lo - o| <= |lo| + |o|.  All of it is below
// 16 x 2^-24 x (|box| + |shift| + |o|), with |.| the largest coordinate magnitude.  The pad is 2^-14 of that sum — a factor of 64 above the
// bound, 6e-5 of the scene's size, far below any emitter's — in two parts: the host's, from the box and the shift (float 3 of the record),
// and the ray's, from its origin.
constexpr float LIGHT_BOX_PAD = 1.0f / 16384.0f;
PT_HD inline float light_box_host_pad(const float lo[3], const float hi[3], const float shift[3]) {
    float m = 0.0f, s = 0.0f;
    for (int a = 0; a < 3; ++a) { m = pe_max(m, pe_max(pe_abs(lo[a]), pe_abs(hi[a]))); s = pe_max(s, pe_abs(shift[a])); }
    return LIGHT_BOX_PAD * (m + s);
}
// The slab test on t >= 0 against the box grown by pad_host + LIGHT_BOX_PAD x max|o|.  Any NaN (0 x inf: an axis-parallel ray whose
// origin lies on the padded face's plane; a NaN origin or direction) answers "may reach".  False positives cost a traced ray, nothing else.
PT_HD inline bool light_box_may_reach(const float o[3], const float d[3], const float lo[3], const float hi[3], float pad_host) {
    if (!(lo[0] <= hi[0])) return false;                                       // the empty box
    const float pad = pad_host + LIGHT_BOX_PAD * pe_max(pe_abs(o[0]), pe_max(pe_abs(o[1]), pe_abs(o[2])));
    if (!(pad == pad)) return true;
    float tn = 0.0f, tf = __builtin_huge_valf();
    for (int a = 0; a < 3; ++a) {
        const float inv = 1.0f / d[a];
        const float t0 = ((lo[a] - pad) - o[a]) * inv, t1 = ((hi[a] + pad) - o[a]) * inv;
        if (!(t0 == t0) || !(t1 == t1)) return true;
        tn = pe_max(tn, pe_min(t0, t1)); tf = pe_min(tf, pe_max(t0, t1));
    }
    return !(tn > tf);
}

// The box records of a light list, from the values the lights' DevLightTri records hold (render-space vertices): what the upload and every
// in-place update (camera re-base, instance move, deformation: scene_update.cpp) write behind the device's light records.  `shift`:
// DevScene::tri_shift's magnitude enters the pad (zeros when the traversals test render-space triangles).
inline void light_boxes(const std::vector<DevLight>& lights, const std::vector<DevLightTri>& light_tris, const float shift[3], std::vector<float>* out) {
    out->assign(lights.size() * LIGHT_BOX_FLOATS, 0.0f);
    for (size_t li = 0; li < lights.size(); ++li) {
        float lo[3] = {1.0f, 1.0f, 1.0f}, hi[3] = {-1.0f, -1.0f, -1.0f};        // empty
        const DevLight& l = lights[li];
        if (l.kind == LK_AREA && l.n_tris != 0u && (size_t)l.first_tri + l.n_tris <= light_tris.size()) {
            for (int a = 0; a < 3; ++a) { lo[a] = __builtin_huge_valf(); hi[a] = -__builtin_huge_valf(); }
            for (uint32_t t = 0; t < l.n_tris; ++t) {
                const DevLightTri& r = light_tris[l.first_tri + t];
                const float v[3][3] = {{r.p0[0], r.p0[1], r.p0[2]}, {r.p1x, r.p1yz[0], r.p1yz[1]}, {r.p2xy[0], r.p2xy[1], r.p2z}};
                for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { lo[a] = pe_min(lo[a], v[k][a]); hi[a] = pe_max(hi[a], v[k][a]); }
            }
        }
        float* b = out->data() + li * LIGHT_BOX_FLOATS;
        b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = (lo[0] <= hi[0]) ? light_box_host_pad(lo, hi, shift) : 0.0f;
        b[4] = hi[0]; b[5] = hi[1]; b[6] = hi[2]; b[7] = 0.0f;
    }
}
// where the boxes live on the device: behind the n_lights light records, in the same allocation (DevScene keeps its size, the lowered light
// records their bytes)
// the whole allocation DevScene::lights names: n_lights records, then n_lights boxes.  The ONE statement of its size: the upload allocates and
// fills it through light_allocation(), the update step and the kernels find the boxes through light_box_of()
inline size_t light_allocation_bytes(size_t n_lights) { return n_lights * (sizeof(DevLight) + LIGHT_BOX_FLOATS * sizeof(float)); }
inline std::vector<unsigned char> light_allocation(const std::vector<DevLight>& lights, const std::vector<DevLightTri>& light_tris, const float shift[3]) {
    std::vector<float> boxes;
    light_boxes(lights, light_tris, shift, &boxes);
    std::vector<unsigned char> bytes(light_allocation_bytes(lights.size()));
    unsigned char* p = bytes.data();
    for (size_t i = 0; i < lights.size() * sizeof(DevLight); ++i) p[i] = ((const unsigned char*)lights.data())[i];
    for (size_t i = 0; i < boxes.size() * sizeof(float); ++i) p[lights.size() * sizeof(DevLight) + i] = ((const unsigned char*)boxes.data())[i];
    return bytes;
}
PT_HD inline const float* light_box_of(const DevLight* lights, uint32_t n_lights, uint32_t li) {
    return (const float*)(lights + n_lights) + (size_t)li * LIGHT_BOX_FLOATS;
}

}  // namespace pt
