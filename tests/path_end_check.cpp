// CPU check of csrc/path_end_plan.hpp (tests/test_path_end.py compiles and runs it; plain g++, -ffp-contract=off like the library).
//
//   path_end_check <seed>
//
// 1. BOX AGAINST TRIANGLES.  Seeded area lights (one to eight triangles: slanted fans, flat axis-aligned quads like a ceiling light, slivers) at
//    coordinates of 1, 10, 600 (the largest the scenes use: the Cornell room in millimetres) and 60 000, each in both vertex forms the traversals
//    test: render space, and "local" vertices with the ray origin shifted (DevScene::tri_shift; render = fl(local + t), the box from the render
//    vertices as light_boxes() makes it from the DevLightTri records).  Rays: at the interior, the edges and the vertices of a triangle, from
//    anywhere in the scene and from the box's own faces (padded and unpadded), axis-parallel directions with +-0 components, rays that graze
//    a flat box nearly in its plane.  Whenever the kernels' watertight test (restated from pt_device.hpp intersect_triangle<false> + setup_ray,
//    as tests/camera_candidates_check.cpp does) hits a triangle of the light, light_box_may_reach must say so: zero misses.  Rays sent past the
//    light say what the test is worth: most of them must be turned away.
// 2. THE DECISION AGAINST THE FRONT.  The roulette and depth statements of shade_vertex_head (pt_path.hpp: the non-emitter term, T *= f / pdf,
//    p = max(T), the draw, the division, the depth test) restated as they stand, on random and adversarial inputs — T with +-0, denormals, inf,
//    NaN; pdf 0 and inf; p exactly at the gate; p = 0; a gate with slack; depth at max_depth and one below.  path_end_draws must say when the
//    front draws, path_end_doomed when it ends the path, the front without the draw (PHASE 4) must leave the survivor's T bit for bit, and
//    path_end_term_is_zero may only be true where adding the term leaves L's bits alone.
// Prints "ok <lights> <rays> <hits> <hits on edges or vertices> <axis-parallel hits> <far rays> <far rays turned away> <decisions> <doomed> <nonzero terms>"
// or the first violation.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "path_end_plan.hpp"

using namespace pt;

struct V { float x, y, z; };
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator*(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float comp(V a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }
static void set_comp(V& a, int k, float v) { (k == 0 ? a.x : k == 1 ? a.y : a.z) = v; }
static V normalize(V a) { const float r = 1.0f / std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return a * r; }
static float max3f(float a, float b, float c) { return std::fmax(a, std::fmax(b, c)); }

// pt_device.hpp intersect_triangle<false> + setup_ray
static bool intersect_triangle(V ro, V rd, V q0, V q1, V q2, float t_max) {
    const float ax = std::fabs(rd.x), ay = std::fabs(rd.y), az = std::fabs(rd.z);
    int kz = 0; float m = ax;
    if (ay > m) { m = ay; kz = 1; }
    if (az > m) { kz = 2; }
    int kx = kz + 1; if (kx == 3) kx = 0;
    int ky = kx + 1; if (ky == 3) ky = 0;
    const float dx = comp(rd, kx), dy = comp(rd, ky), dz = comp(rd, kz);
    const float sx = -dx / dz, sy = -dy / dz, sz = 1.0f / dz;
    V a0 = q0 - ro, a1 = q1 - ro, a2 = q2 - ro;
    float p0x = comp(a0, kx), p0y = comp(a0, ky), p0z = comp(a0, kz);
    float p1x = comp(a1, kx), p1y = comp(a1, ky), p1z = comp(a1, kz);
    float p2x = comp(a2, kx), p2y = comp(a2, ky), p2z = comp(a2, kz);
    p0x += sx * p0z; p0y += sy * p0z;
    p1x += sx * p1z; p1y += sy * p1z;
    p2x += sx * p2z; p2y += sy * p2z;
    float e0 = p2x * p1y - p2y * p1x;
    float e1 = p0x * p2y - p0y * p2x;
    float e2 = p1x * p0y - p1y * p0x;
    if (e0 == 0.0f || e1 == 0.0f || e2 == 0.0f) {
        e0 = (float)((double)p2x * (double)p1y - (double)p2y * (double)p1x);
        e1 = (float)((double)p0x * (double)p2y - (double)p0y * (double)p2x);
        e2 = (float)((double)p1x * (double)p0y - (double)p1y * (double)p0x);
    }
    if ((e0 < 0.0f || e1 < 0.0f || e2 < 0.0f) && (e0 > 0.0f || e1 > 0.0f || e2 > 0.0f)) return false;
    const float det = e0 + e1 + e2;
    if (det == 0.0f) return false;
    p0z *= sz; p1z *= sz; p2z *= sz;
    const float t_scaled = e0 * p0z + e1 * p1z + e2 * p2z;
    if (det < 0.0f && (t_scaled >= 0.0f || t_scaled < t_max * det)) return false;
    if (det > 0.0f && (t_scaled <= 0.0f || t_scaled > t_max * det)) return false;
    const float inv_det = 1.0f / det;
    const float t_hit = t_scaled * inv_det;
    constexpr float EPSH = 1.1920929e-7f * 0.5f;
    constexpr float G2 = (2.0f * EPSH) / (1.0f - 2.0f * EPSH), G3 = (3.0f * EPSH) / (1.0f - 3.0f * EPSH), G5 = (5.0f * EPSH) / (1.0f - 5.0f * EPSH);
    const float max_zt = max3f(std::fabs(p0z), std::fabs(p1z), std::fabs(p2z));
    const float delta_z = G3 * max_zt;
    const float max_xt = max3f(std::fabs(p0x), std::fabs(p1x), std::fabs(p2x));
    const float max_yt = max3f(std::fabs(p0y), std::fabs(p1y), std::fabs(p2y));
    const float delta_x = G5 * max_xt, delta_y = G5 * max_yt;
    const float delta_e = 2.0f * (G2 * max_xt * max_yt + delta_y * max_xt + delta_x * max_yt);
    const float max_e = max3f(std::fabs(e0), std::fabs(e1), std::fabs(e2));
    const float delta_t = 3.0f * (G3 * max_e * max_zt + delta_e * max_zt + delta_z * max_e) * std::fabs(inv_det);
    if (t_hit < delta_t) return false;
    return true;
}

static int fail(const char* what, const char* detail) { std::printf("FAIL %s: %s\n", what, detail); return 1; }

struct Counts { unsigned long long lights = 0, rays = 0, hits = 0, edge_hits = 0, axis_hits = 0, far = 0, far_away = 0, decisions = 0, doomed = 0, nonzero = 0; };

struct Light {
    std::vector<V> local, render;       // 3 per triangle
    V t;                                // render = fl(local + t); the traversal's shift is -t
    bool shifted;
    float lo[3], hi[3], pad;            // the box record
};

static std::mt19937 rng;
static float uni(float a, float b) { return a + (b - a) * (float)(rng() >> 8) * (1.0f / 16777216.0f); }

static Light make_light(float scale, int kind, bool shifted) {
    Light L;
    L.shifted = shifted;
    L.t = shifted ? V{uni(-scale, scale), uni(-scale, scale), uni(-scale, scale)} : V{0, 0, 0};
    const V c{uni(-scale, scale) * 0.8f, uni(-scale, scale) * 0.8f, uni(-scale, scale) * 0.8f};
    const float ext = scale * uni(0.02f, 0.3f);
    const int n_tri = kind == 1 ? 2 : 1 + (int)(rng() % 8u);
    std::vector<V> render;
    if (kind == 1) {                                       // a flat axis-aligned quad: the box has no thickness but its pad
        const int a = (int)(rng() % 3u), b = (a + 1) % 3, cax = (a + 2) % 3;
        V q[4];
        for (int k = 0; k < 4; ++k) { q[k] = c; set_comp(q[k], b, comp(c, b) + ((k & 1) ? ext : -ext)); set_comp(q[k], cax, comp(c, cax) + ((k & 2) ? ext : -ext)); }
        render = {q[0], q[1], q[3], q[0], q[3], q[2]};
    } else {
        for (int i = 0; i < n_tri; ++i) {
            V p0{c.x + uni(-ext, ext), c.y + uni(-ext, ext), c.z + uni(-ext, ext)};
            const float e = kind == 2 ? ext * 1e-4f : ext;   // slivers
            V p1{p0.x + uni(-ext, ext), p0.y + uni(-e, e), p0.z + uni(-ext, ext)}, p2{p0.x + uni(-ext, ext), p0.y + uni(-e, e), p0.z + uni(-e, e)};
            render.push_back(p0); render.push_back(p1); render.push_back(p2);
        }
    }
    // the library's order: local vertices are the description's, render = xform_point(local) = fl(local + t)
    for (const V& r : render) { const V l = r - L.t; L.local.push_back(l); L.render.push_back(l + L.t); }
    // the box through light_boxes(), from DevLightTri records
    std::vector<DevLight> lights(2);
    std::vector<DevLightTri> tris(L.render.size() / 3);
    lights[0] = DevLight{}; lights[0].kind = LK_POINT;                         // a delta light ahead of it: an empty box
    lights[1] = DevLight{}; lights[1].kind = LK_AREA; lights[1].first_tri = 0; lights[1].n_tris = (uint32_t)tris.size();
    for (size_t i = 0; i < tris.size(); ++i) {
        const V p0 = L.render[3 * i], p1 = L.render[3 * i + 1], p2 = L.render[3 * i + 2];
        DevLightTri r{};
        r.p0[0] = p0.x; r.p0[1] = p0.y; r.p0[2] = p0.z; r.p1x = p1.x; r.p1yz[0] = p1.y; r.p1yz[1] = p1.z; r.p2xy[0] = p2.x; r.p2xy[1] = p2.y; r.p2z = p2.z;
        tris[i] = r;
    }
    const float shift[3] = {-L.t.x, -L.t.y, -L.t.z};
    std::vector<float> boxes;
    light_boxes(lights, tris, shift, &boxes);
    const float* b = boxes.data() + LIGHT_BOX_FLOATS;
    for (int a = 0; a < 3; ++a) { L.lo[a] = b[a]; L.hi[a] = b[4 + a]; }
    L.pad = b[3];
    return L;
}

static bool empty_box_is_never_reached() {
    std::vector<DevLight> lights(1); lights[0] = DevLight{}; lights[0].kind = LK_SPOT;
    std::vector<DevLightTri> none;
    const float z[3] = {0, 0, 0};
    std::vector<float> boxes;
    light_boxes(lights, none, z, &boxes);
    const float o[3] = {0, 0, 0}, d[3] = {0, 0, 1}, nan_d[3] = {NAN, 0, 1};
    return !light_box_may_reach(o, d, boxes.data(), boxes.data() + 4, boxes[3]) && !light_box_may_reach(o, nan_d, boxes.data(), boxes.data() + 4, boxes[3]);
}

// one ray against the light: returns false on a miss of the box test where a triangle is hit
static bool check_ray(const Light& L, V o, V d, Counts& n, unsigned long long* class_hits) {
    ++n.rays;
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    const bool reach = light_box_may_reach(oo, dd, L.lo, L.hi, L.pad);
    bool hit = false;
    for (size_t i = 0; i + 2 < L.render.size() && !hit; i += 3) {
        // both forms, whichever the scene would use: the box must hold for either
        hit = intersect_triangle(o, d, L.render[i], L.render[i + 1], L.render[i + 2], FLT_MAX);
        if (!hit && L.shifted) hit = intersect_triangle(o - L.t, d, L.local[i], L.local[i + 1], L.local[i + 2], FLT_MAX);
    }
    if (hit) { ++n.hits; if (class_hits) ++*class_hits; }
    if (hit && !reach) {
        std::printf("FAIL box: a ray that hits the light is turned away: o = (%.9g %.9g %.9g) d = (%.9g %.9g %.9g) box (%.9g %.9g %.9g) .. (%.9g %.9g %.9g) pad %.9g\n",
                    o.x, o.y, o.z, d.x, d.y, d.z, L.lo[0], L.lo[1], L.lo[2], L.hi[0], L.hi[1], L.hi[2], L.pad);
        return false;
    }
    return true;
}

static bool check_boxes(Counts& n) {
    const float scales[4] = {1.0f, 10.0f, 600.0f, 60000.0f};
    for (int si = 0; si < 4; ++si) for (int kind = 0; kind < 3; ++kind) for (int shifted = 0; shifted < 2; ++shifted) for (int rep = 0; rep < 6; ++rep) {
        const float S = scales[si];
        const Light L = make_light(S, kind, shifted != 0);
        ++n.lights;
        const size_t n_tri = L.render.size() / 3;
        for (int r = 0; r < 600; ++r) {
            const size_t ti = rng() % n_tri;
            const V p0 = L.render[3 * ti], p1 = L.render[3 * ti + 1], p2 = L.render[3 * ti + 2];
            // the target: interior, an edge, a vertex
            float b0 = uni(0, 1), b1 = uni(0, 1);
            if (b0 + b1 > 1.0f) { b0 = 1.0f - b0; b1 = 1.0f - b1; }
            const int where = r % 4;
            if (where == 1) b1 = 0.0f;
            if (where == 2) { b0 = (r & 4) ? 1.0f : 0.0f; b1 = (r & 8) ? 0.0f : 1.0f - b0; }
            const V target = p0 * (1.0f - b0 - b1) + p1 * b0 + p2 * b1;
            // the origin: anywhere in the scene; on a face plane of the box, unpadded or padded; nearly in the plane of a flat box, far out
            V o{uni(-S, S), uni(-S, S), uni(-S, S)};
            const int from = (r / 4) % 5;
            if (from == 1 || from == 2) {
                const int a = (int)(rng() % 3u);
                const float pad_all = L.pad + LIGHT_BOX_PAD * max3f(std::fabs(o.x), std::fabs(o.y), std::fabs(o.z));
                const bool low = (rng() & 1u) != 0u;
                set_comp(o, a, from == 1 ? (low ? L.lo[a] : L.hi[a]) : (low ? L.lo[a] - pad_all : L.hi[a] + pad_all));
            }
            if (from == 3 && kind == 1) {
                for (int a = 0; a < 3; ++a) if (L.lo[a] == L.hi[a]) set_comp(o, a, L.lo[a] + uni(-1.0f, 1.0f) * S * 1e-6f);
            }
            V d = target - o;
            if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) continue;
            unsigned long long* cls = where != 0 ? &n.edge_hits : nullptr;
            if (from == 4) {
                // axis-parallel: the origin straight above / below / beside the target, the other components +0 or -0
                const int a = (int)(rng() % 3u);
                o = target; set_comp(o, a, comp(target, a) + ((rng() & 1u) ? 1.0f : -1.0f) * S * uni(0.01f, 1.5f));
                d = V{(rng() & 1u) ? 0.0f : -0.0f, (rng() & 2u) ? 0.0f : -0.0f, (rng() & 4u) ? 0.0f : -0.0f};
                set_comp(d, a, comp(target, a) - comp(o, a) > 0.0f ? 1.0f : -1.0f);
                cls = &n.axis_hits;
            } else if (r & 1) d = normalize(d);
            if (!check_ray(L, o, d, n, cls)) return false;
        }
        // rays sent past the light: at points four box diagonals away from it
        for (int r = 0; r < 200; ++r) {
            const V o{uni(-S, S), uni(-S, S), uni(-S, S)};
            const float ext = max3f(L.hi[0] - L.lo[0], L.hi[1] - L.lo[1], L.hi[2] - L.lo[2]);
            const int a = (int)(rng() % 3u);
            V target{uni(L.lo[0], L.hi[0]), uni(L.lo[1], L.hi[1]), uni(L.lo[2], L.hi[2])};
            set_comp(target, a, comp(target, a) + ((rng() & 1u) ? 4.0f : -4.0f) * ext);
            const V away = target - o;
            // (only rays whose origin is on the far side of the displaced target plane can be told apart for sure; count what the test does)
            const float oo[3] = {o.x, o.y, o.z}, dd[3] = {away.x, away.y, away.z};
            ++n.far;
            if (!light_box_may_reach(oo, dd, L.lo, L.hi, L.pad)) ++n.far_away;
            if (!check_ray(L, o, normalize(away), n, nullptr)) return false;
        }
    }
    return true;
}

// ---- 2. the decision ----
static float balance_heuristic(float a, float b) { return (a == 0.0f && b == 0.0f) ? 0.0f : a / (a + b); }
static uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

struct Front { bool drew, end_path; float T[4], term[4]; bool term_added; uint32_t depth; };
// shade_vertex_head, PHASE 3, a hit that is no emitter, not a camera ray: the statements from the non-emitter term to the depth test
static Front front(const float T_in[4], const float pf[4], float p_pdf, float ur, float rr_gate, uint32_t depth, uint32_t max_depth, uint32_t strategy, bool prev_spec) {
    Front f{};
    float T[4] = {T_in[0], T_in[1], T_in[2], T_in[3]};
    bool end_path = false;
    const float tf = 1.0f / p_pdf;
    if (strategy != 1u || prev_spec) {
        const float w = (strategy == 2u && !prev_spec) ? balance_heuristic(p_pdf, 0.0f) : 1.0f;
        for (int i = 0; i < 4; ++i) f.term[i] = (T[i] * 0.0f) * w;
        f.term_added = true;
    }
    for (int i = 0; i < 4; ++i) T[i] = T[i] * (pf[i] * tf);
    const float p = fmaxf(fmaxf(fmaxf(fmaxf(-INFINITY, T[0]), T[1]), T[2]), T[3]);
    if (!(p >= rr_gate)) {
        f.drew = true;
        if (ur < p) {
            if (p != 0.0f) for (int i = 0; i < 4; ++i) T[i] = T[i] / p;
        } else end_path = true;
    }
    if (!end_path) {
        depth += 1;
        if (depth > max_depth) end_path = true;
    }
    f.end_path = end_path; f.depth = depth;
    for (int i = 0; i < 4; ++i) f.T[i] = T[i];
    return f;
}
// shade_vertex_head, PHASE 4: the same front without the draw, for a path that carries the decision
static void front_no_draw(const float T_in[4], const float pf[4], float p_pdf, float rr_gate, bool doomed, float T[4], bool* end_path) {
    const float tf = 1.0f / p_pdf;
    for (int i = 0; i < 4; ++i) T[i] = T_in[i] * (pf[i] * tf);
    const float p = fmaxf(fmaxf(fmaxf(fmaxf(-INFINITY, T[0]), T[1]), T[2]), T[3]);
    *end_path = false;
    if (doomed) *end_path = true;
    else if (!(p >= rr_gate) && p != 0.0f) for (int i = 0; i < 4; ++i) T[i] = T[i] / p;
}

static bool check_one(const float T[4], const float pf[4], float p_pdf, float ur, float gate, uint32_t depth, uint32_t max_depth, uint32_t strategy, bool prev_spec, Counts& n) {
    ++n.decisions;
    const Front f = front(T, pf, p_pdf, ur, gate, depth, max_depth, strategy, prev_spec);
    const float p = path_end_pmax(T, pf, p_pdf);
    const bool draws = path_end_draws(p, gate);
    const bool doomed = path_end_doomed(p, draws ? ur : 123.0f, gate, depth, max_depth);       // (the draw is not read when none is made)
    char msg[512];
    std::snprintf(msg, sizeof msg, "T = (%.9g %.9g %.9g %.9g) pf = (%.9g %.9g %.9g %.9g) pdf %.9g ur %.9g gate %.9g depth %u / %u strategy %u spec %d", T[0], T[1], T[2], T[3],
                  pf[0], pf[1], pf[2], pf[3], p_pdf, ur, gate, depth, max_depth, strategy, (int)prev_spec);
    if (draws != f.drew) return fail("the draw is made where the front makes none, or the other way round", msg) == 0;
    if (doomed != f.end_path) return fail("doomed differs from the front's end of the path", msg) == 0;
    if (doomed) ++n.doomed;
    float T4[4]; bool end4;
    front_no_draw(T, pf, p_pdf, gate, doomed, T4, &end4);
    if (end4 != f.end_path) return fail("the front without the draw ends another path", msg) == 0;
    if (!end4) for (int i = 0; i < 4; ++i) if (bits_of(T4[i]) != bits_of(f.T[i])) return fail("the survivor's throughput differs", msg) == 0;
    // the term
    if (f.term_added) {
        const float w = (strategy == 2u && !prev_spec) ? balance_heuristic(p_pdf, 0.0f) : 1.0f;
        const bool zero = path_end_term_is_zero(T, w);
        bool leaves_L = true;
        const float Ls[4] = {0.0f, 1.5f, 3.0e-41f, 7.0e37f};
        for (int i = 0; i < 4; ++i) for (float L0 : Ls) if (bits_of(L0 + f.term[i]) != bits_of(L0)) leaves_L = false;
        if (!leaves_L) ++n.nonzero;
        if (zero && !leaves_L) return fail("a skip is allowed where the term changes L", msg) == 0;
        if (!zero && leaves_L) return fail("a term that is an exact zero is not seen as one", msg) == 0;
    }
    return true;
}

static bool check_decisions(Counts& n) {
    const float sp[] = {0.0f, -0.0f, 1.4e-45f, 1.0e-40f, FLT_MIN, 0.25f, 0.5f, 0.99999994f, 1.0f, 1.0000001f, 2.0f, 1.0e30f, FLT_MAX, INFINITY, -INFINITY, NAN, -1.0f};
    const float pdfs[] = {0.0f, -0.0f, 1.0e-40f, 1.0e-30f, 0.5f, 1.0f, 3.0f, 1.0e30f, INFINITY, NAN};
    const float gates[] = {1.0f, 0.75f, 0.99f};
    const uint32_t depths[][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 2}, {2, 2}, {5, 16}, {15, 16}, {16, 16}, {999, 1000}, {1000, 1000}};
    const int n_sp = (int)(sizeof sp / sizeof sp[0]);
    // adversarial: every special value as the dominant throughput, against every pdf, gate, depth pair, strategy
    for (int a = 0; a < n_sp; ++a) for (int b = 0; b < n_sp; ++b) for (float pdf : pdfs) for (float gate : gates) for (const auto& dm : depths) for (uint32_t strategy = 0; strategy < 3; ++strategy) {
        const float T[4] = {sp[a], sp[b], sp[(a + b) % n_sp], 0.5f};
        const float pf[4] = {1.0f, sp[(a * 7 + 3) % n_sp], 0.5f, 1.0f};
        const float p = path_end_pmax(T, pf, pdf);
        // the draw at, just below and just above p, and at the ends of [0, 1)
        const float urs[] = {0.0f, 0.99999994f, p, std::nextafterf(p, -INFINITY), std::nextafterf(p, INFINITY), 0.5f};
        for (float ur : urs) if (!check_one(T, pf, pdf, ur, gate, dm[0], dm[1], strategy, ((a + b) & 1) != 0, n)) return false;
    }
    // p exactly at the gate, and p == 0
    for (float gate : gates) for (const auto& dm : depths) {
        const float T[4] = {gate, 0.25f, 0.0f, gate}, one[4] = {1, 1, 1, 1}, zero[4] = {0, 0, 0, 0};
        for (float ur : {0.0f, 0.5f, std::nextafterf(gate, 0.0f), gate})
            if (!check_one(T, one, 1.0f, ur, gate, dm[0], dm[1], 2u, false, n) || !check_one(zero, one, 1.0f, ur, gate, dm[0], dm[1], 2u, false, n) ||
                !check_one(T, zero, 1.0f, ur, gate, dm[0], dm[1], 1u, true, n)) return false;
    }
    // random
    for (int i = 0; i < 100000; ++i) {
        float T[4], pf[4];
        for (int k = 0; k < 4; ++k) { T[k] = uni(0.0f, 1.2f) * ((rng() % 16u) ? 1.0f : 0.0f); pf[k] = uni(0.0f, 1.0f); }
        const float pdf = (rng() % 64u) ? uni(0.01f, 2.0f) : 0.0f;
        const auto& dm = depths[rng() % 10u];
        if (!check_one(T, pf, pdf, uni(0.0f, 1.0f), gates[rng() % 3u], dm[0], dm[1], rng() % 3u, (rng() & 1u) != 0u, n)) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <seed>\n", argv[0]); return 2; }
    rng.seed((uint32_t)std::strtoul(argv[1], nullptr, 10));
    Counts n;
    if (!empty_box_is_never_reached()) return fail("box", "the empty box of a light that is no area light is reached");
    if (!check_boxes(n)) return 1;
    if (!check_decisions(n)) return 1;
    std::printf("ok %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", n.lights, n.rays, n.hits, n.edge_hits, n.axis_hits, n.far, n.far_away, n.decisions, n.doomed, n.nonzero);
    return 0;
}
