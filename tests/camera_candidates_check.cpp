// CPU check of csrc/camera_candidates.hpp (tests/test_camera_candidates.py compiles and runs it; plain g++, -ffp-contract=off like the library).
//
//   camera_candidates_check <seed> <n_tris> <frame_w> <frame_h> [<dir_x> <dir_y> <dir_z> <up_x> <up_y> <up_z> <fov_deg>]
//
// Builds a seeded synthetic scene — random triangles all round the render-space origin (in front of the camera, behind it, straddling the
// pyramids' side planes, a few large ones whose boxes contain the apex), a 4-wide tree over them with 1 .. 3 triangles per leaf, 2 .. 4 children
// per node, unused slots as point boxes at +FLT_MAX and every box padded like the lowered tree's — and a random camera, or, with the seven
// optional arguments, the camera launch_plan.hpp make_camera builds from that direction, up and field of view (tests/camera_cases.py: rolled,
// along an axis, 1 to 170 degrees wide; the scene of the seed stays the same).  For a set of pixel
// rectangles (frame corners, frame edges, interior; 1x1 up to 8x8) it walks the tree with the header and shoots camera rays with
// regen_path's arithmetic through the rectangle's corners, edges and interior.  Every triangle a brute-force loop of the kernels' watertight
// test (restated below from pt_device.hpp intersect_triangle<false>, limit FLT_MAX) hits must be in the rectangle's list.  With the exact
// count K of a rectangle known, a walk with cap = K must return all K without overflow and a walk with cap = K - 1 must report overflow.
// Prints "ok <rects> <rays> <hits> <longest list> <lists with triangles culled by the behind plane> <leaf slots unused>" or the first violation.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "camera_candidates.hpp"
#include "launch_plan.hpp"

using namespace pt;

struct V { float x, y, z; };
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator*(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float comp(V a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }
static V normalize(V a) { const float r = 1.0f / std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return a * r; }
static V cross(V a, V b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
static float max3f(float a, float b, float c) { return std::fmax(a, std::fmax(b, c)); }

// pt_device.hpp intersect_triangle<false> + setup_ray
static bool intersect_triangle(V ro, V rd, V q0, V q1, V q2, float t_max, float& t_out) {
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
    t_out = t_hit;
    return true;
}

// pt_path.hpp regen_path: the camera ray through (fx, fy) = pixel + pixel sample
static void camera_ray(const DevCamera& cam, uint32_t px, uint32_t py, float ux, float uy, V& ro, V& rd) {
    const float fx = (float)px + (ux * 1.0f - 1.0f * 0.5f) + 0.5f, fy = (float)py + (uy * 1.0f - 1.0f * 0.5f) + 0.5f;
    const float dx = (2.0f * fx / (float)cam.width - 1.0f) * cam.aspect * cam.tan_half_fov;
    const float dy = (1.0f - 2.0f * fy / (float)cam.height) * cam.tan_half_fov;
    const V dc = normalize(V{dx, dy, -1.0f});
    const V s{cam.s[0], cam.s[1], cam.s[2]}, u{cam.u[0], cam.u[1], cam.u[2]}, f{cam.f[0], cam.f[1], cam.f[2]};
    rd = normalize(s * dc.x + u * dc.y + (f * -1.0f) * dc.z);
    ro = V{0, 0, 0} + rd * 1e-5f;                                           // RAY_EPS
}

struct Box { float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}; };
static void grow(Box& b, const float* p) { for (int a = 0; a < 3; ++a) { b.lo[a] = std::min(b.lo[a], p[a]); b.hi[a] = std::max(b.hi[a], p[a]); } }

struct Builder {
    std::vector<DevTri>& tris;            // reordered into leaf order
    std::vector<DevNode4> nodes;
    std::mt19937& rng;
    float pad;
    uint32_t unused_slots = 0;
    Box bounds(uint32_t b, uint32_t e) const {
        Box x;
        for (uint32_t i = b; i < e; ++i) { const float* p = (const float*)&tris[i]; grow(x, p); grow(x, p + 3); grow(x, p + 6); }
        for (int a = 0; a < 3; ++a) { x.lo[a] -= pad; x.hi[a] += pad; }
        return x;
    }
    int32_t build(uint32_t b, uint32_t e) {                                  // link of the subtree over tris [b, e)
        const uint32_t n = e - b;
        if (n <= 1u + rng() % 3u) return make_leaf(b, n);
        Box x = bounds(b, e);
        int axis = 0; for (int a = 1; a < 3; ++a) if (x.hi[a] - x.lo[a] > x.hi[axis] - x.lo[axis]) axis = a;
        std::sort(tris.begin() + b, tris.begin() + e, [&](const DevTri& p, const DevTri& q) { return ((const float*)&p)[axis] < ((const float*)&q)[axis]; });
        const uint32_t k = std::min<uint32_t>(2u + rng() % 3u, n);           // 2 .. 4 children
        const int32_t idx = (int32_t)nodes.size();
        nodes.push_back(DevNode4{});
        DevNode4 d{};
        for (uint32_t c = 0; c < 4u; ++c) {
            if (c < k) {
                const uint32_t cb = b + (uint32_t)((uint64_t)n * c / k), ce = b + (uint32_t)((uint64_t)n * (c + 1) / k);
                const Box cx = bounds(cb, ce);
                d.lox[c] = cx.lo[0]; d.loy[c] = cx.lo[1]; d.loz[c] = cx.lo[2]; d.hix[c] = cx.hi[0]; d.hiy[c] = cx.hi[1]; d.hiz[c] = cx.hi[2];
                d.child[c] = build(cb, ce);
            } else {
                d.lox[c] = d.loy[c] = d.loz[c] = d.hix[c] = d.hiy[c] = d.hiz[c] = FLT_MAX; d.child[c] = 0; ++unused_slots;
            }
        }
        nodes[(size_t)idx] = d;
        return idx;
    }
};

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc != 5 && argc != 12) {
        std::fprintf(stderr, "usage: %s <seed> <n_tris> <frame_w> <frame_h> [<dir_x> <dir_y> <dir_z> <up_x> <up_y> <up_z> <fov_deg>]\n", argv[0]);
        return 2;
    }
    const uint32_t seed = (uint32_t)std::atoi(argv[1]), n_tris = (uint32_t)std::atoi(argv[2]), W = (uint32_t)std::atoi(argv[3]), H = (uint32_t)std::atoi(argv[4]);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    auto sym = [&](float r) { return (2.0f * U(rng) - 1.0f) * r; };

    // the camera: a random orthonormal basis the way launch_plan.hpp make_camera builds it
    DevCamera cam{};
    {
        const V f = normalize(V{sym(1.0f), sym(1.0f), sym(1.0f) - 1.5f}), up = normalize(V{sym(0.3f), 1.0f, sym(0.3f)});
        const V s = normalize(cross(f, up)), u = cross(s, f);
        cam.s[0] = s.x; cam.s[1] = s.y; cam.s[2] = s.z; cam.u[0] = u.x; cam.u[1] = u.y; cam.u[2] = u.z; cam.f[0] = f.x; cam.f[1] = f.y; cam.f[2] = f.z;
        cam.tan_half_fov = std::tan((30.0f + 60.0f * U(rng)) * 0.5f * 3.14159265f / 180.0f);
        cam.aspect = (float)W / (float)H; cam.width = W; cam.height = H;
    }
    if (argc == 12) {                                                      // (after the random one, so that the seed's scene does not change)
        mi355pt_camera c{};
        for (int a = 0; a < 3; ++a) { c.direction[a] = (float)std::atof(argv[5 + a]); c.up[a] = (float)std::atof(argv[8 + a]); }
        c.fov_deg = (float)std::atof(argv[11]); c.width = W; c.height = H;
        cam = make_camera(&c);
    }
    // triangles all round the origin: small ones at every distance, every 16th a large one (its box may contain the apex)
    std::vector<DevTri> tris(n_tris);
    const float shift[3] = {sym(4.0f), sym(4.0f), sym(4.0f)};            // DevScene::tri_shift: the array holds vertices + shift
    const bool local = (seed & 1u) != 0u;
    for (uint32_t i = 0; i < n_tris; ++i) {
        const bool large = i % 16u == 0u;
        const float dist = large ? 6.0f * U(rng) : 0.05f + 12.0f * U(rng) * U(rng), size = large ? 8.0f : 0.02f + 0.8f * U(rng);
        const V c = normalize(V{sym(1.0f), sym(1.0f), sym(1.0f) + 1e-3f}) * dist;
        float* p = (float*)&tris[i];
        for (int v = 0; v < 3; ++v) { p[3 * v] = c.x + sym(size); p[3 * v + 1] = c.y + sym(size); p[3 * v + 2] = c.z + sym(size); }
        tris[i].instance = 0; tris[i].flags = 0; tris[i].mclass = 0;
    }
    float R = 0.0f;
    for (const DevTri& t : tris) for (int k = 0; k < 9; ++k) R = std::max(R, std::fabs(((const float*)&t)[k]));
    Builder b{tris, {}, rng, NODE4_PAD_REL * R};
    const int32_t root4 = b.build(0, n_tris);
    if (root4 < 0) FAIL("the tree has no node");
    // (render-space vertices in `tris`; the array the walk and the test read holds them shifted when the scene is `local`)
    std::vector<DevTri> arr = tris;
    float tri_shift[3] = {0, 0, 0};
    if (local) for (int a = 0; a < 3; ++a) tri_shift[a] = shift[a];
    for (DevTri& t : arr) { float* p = (float*)&t; for (int v = 0; v < 3; ++v) for (int a = 0; a < 3; ++a) p[3 * v + a] += tri_shift[a]; }

    struct Rect { uint32_t x0, y0, x1, y1; };
    std::vector<Rect> rects = {{0, 0, 0, 0}, {W - 1, H - 1, W - 1, H - 1}, {0, H - 1, 0, H - 1}, {W - 1, 0, W - 1, 0}, {0, 0, 1, 1}, {W - 2, H - 2, W - 1, H - 1},
                               {W - 8, 0, W - 1, 7}, {0, H / 2, 3, H / 2 + 3}, {W / 2, H / 2, W / 2 + 1, H / 2 + 1}, {W / 2 - 4, H / 2 - 4, W / 2 + 3, H / 2 + 3}};
    for (int i = 0; i < 40; ++i) {
        const uint32_t bs = 1u << (rng() % 4u);
        const uint32_t x0 = (rng() % ((W + bs - 1) / bs)) * bs, y0 = (rng() % ((H + bs - 1) / bs)) * bs;
        rects.push_back({x0, y0, x0 + bs - 1, y0 + bs - 1});               // (may stick out of a ragged frame, like a work item's block)
    }
    const float edge[5] = {0.0f, 0.99999994f, 0.5f, 0.25f, 0.75f};           // pixel samples: u in [0, 1)
    std::vector<uint32_t> list(n_tris + 1u), list2(n_tris + 1u);
    uint32_t stack[CAM_WALK_STACK];
    unsigned long long rays = 0, hits = 0, longest = 0, behind_lists = 0;
    for (const Rect& r : rects) {
        const CamPyramid py = cam_pyramid(cam, r.x0, r.y0, r.x1, r.y1);
        const CamWalk w = cam_walk(b.nodes.data(), root4, arr.data(), tri_shift, py, list.data(), n_tris, stack);
        if (w.overflow || w.count > n_tris) FAIL("rect %u %u %u %u: overflow with cap = all triangles", r.x0, r.y0, r.x1, r.y1);
        std::vector<uint8_t> in(n_tris, 0);
        for (uint32_t i = 0; i < w.count; ++i) { if (list[i] >= n_tris || in[list[i]]) FAIL("index out of range or listed twice"); in[list[i]] = 1; }
        longest = std::max<unsigned long long>(longest, w.count);
        // the cap reached exactly, and exceeded by one
        const CamWalk we = cam_walk(b.nodes.data(), root4, arr.data(), tri_shift, py, list2.data(), w.count, stack);
        if (we.overflow || we.count != w.count || !std::equal(list.begin(), list.begin() + w.count, list2.begin())) FAIL("cap == count must give the whole list");
        if (w.count > 0) {
            const uint32_t guard = list2[w.count - 1];
            const CamWalk wo = cam_walk(b.nodes.data(), root4, arr.data(), tri_shift, py, list2.data(), w.count - 1u, stack);
            if (!wo.overflow || wo.count > w.count - 1u) FAIL("cap == count - 1 must report overflow");
            if (list2[w.count - 1] != guard) FAIL("a walk wrote past its cap");
        }
        // something behind the camera must have been culled by the fifth plane alone (all four side planes pass through the apex: the
        // mirror image of a triangle inside the pyramid is inside all four)
        {
            bool any = false;
            for (uint32_t i = 0; i < n_tris && !any; ++i) {
                if (in[i]) continue;
                const float* p = (const float*)&tris[i];
                Box x; grow(x, p); grow(x, p + 3); grow(x, p + 6);
                CamPyramid sides = py;
                for (int a = 0; a < 3; ++a) sides.n[4][a] = 0.0f;
                sides.n1[4] = 0.0f;
                // (with the fifth normal zeroed its test reads 0 > 0: never outside)
                any = !cam_box_outside(sides, x.lo, x.hi, R) && cam_box_outside(py, x.lo, x.hi, R);
            }
            behind_lists += any ? 1u : 0u;
        }
        // rays through corners, edges and interior of every pixel of the rectangle's border and of some inside
        for (uint32_t py_ = r.y0; py_ <= r.y1; ++py_) for (uint32_t px = r.x0; px <= r.x1; ++px) {
            if (px >= W || py_ >= H) continue;
            for (int iu = 0; iu < 5; ++iu) for (int iv = 0; iv < 5; ++iv) {
                V ro, rd;
                camera_ray(cam, px, py_, edge[iu], edge[iv], ro, rd);
                const V o2 = ro + V{tri_shift[0], tri_shift[1], tri_shift[2]};                  // tri_origin
                ++rays;
                for (uint32_t i = 0; i < n_tris; ++i) {
                    const float* p = (const float*)&arr[i];
                    float t;
                    if (!intersect_triangle(o2, rd, V{p[0], p[1], p[2]}, V{p[3], p[4], p[5]}, V{p[6], p[7], p[8]}, 3.402823466e+38f, t)) continue;
                    ++hits;
                    if (!in[i]) FAIL("rect %u %u %u %u pixel %u %u sample %g %g: triangle %u hit at t = %g but not in the list of %u", r.x0, r.y0, r.x1, r.y1, px,
                                     py_, (double)edge[iu], (double)edge[iv], i, (double)t, w.count);
                }
            }
        }
    }
    std::printf("ok %zu %llu %llu %llu %llu %u\n", rects.size(), rays, hits, longest, behind_lists, b.unused_slots);
    return 0;
}
