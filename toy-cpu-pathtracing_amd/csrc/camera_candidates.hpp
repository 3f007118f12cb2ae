// Camera-ray candidates of a work item (pt_kernel_body.inc): the triangles a camera ray through a rectangle of pixels can hit, found ONCE
// for the rectangle instead of by one tree traversal per ray.  Plain arithmetic on layout.hpp's records — no HIP header, no state — so that
// tests/test_camera_candidates.py runs the walk on the CPU (tests/camera_candidates_check.cpp) and the kernels call the same functions.
//
// Every camera ray of the pixels [x0, x1] x [y0, y1] leaves the render-space origin in a direction s * dx + u * dy + f (regen_path's
// arithmetic before its two normalisations, which scale by a positive factor) with dx, dy inside the rectangle's range, so every point
// rd * (RAY_EPS + t), t >= 0, of every such ray lies inside the PYRAMID with its apex at the origin and four side planes through the
// rectangle's edges, in front of the apex.  A triangle whose box (the padded DevNode4 plane set that holds it: the box the traversal itself
// tests) lies wholly outside one of those five planes cannot be hit by any of the rays, and neither can one whose own bounds do.
// cam_walk() collects the triangles that pass both tests: a superset of what any of the item's camera rays hits, in no particular order
// — the closest hit is a minimum over the set.
//
// ERROR BOUND.  A box is tested against a plane n through the origin by the smallest n . p over its corners, m = sum over axes of
// min(n_a * lo_a, n_a * hi_a): three products and two additions in f32, each rounding by at most u = 2^-24 relative, on terms no larger
// than |n|_1 * R (R = the largest coordinate magnitude of the tree's boxes): |m - exact| <= 3 u |n|_1 R.  The box counts as outside only when
// m > CAM_SLACK_REL * |n|_1 * R with CAM_SLACK_REL = 2^-20 = 16 u, five times that bound.  What rounding does to the planes THEMSELVES (dx, dy,
// the basis not being orthonormal to the last bit, regen_path's own roundings of a direction: all relative errors of a few u of a direction
// component) is covered by the rectangle's margin, CAM_MARGIN_PIX = 1/8 pixel on each side: at 16 384 pixels across a 90-degree view that is
// 1.5e-5 of the direction's length, a hundred times those errors.  The DevNode4 boxes are already padded by 2^-22 R (layout.hpp NODE4_PAD_REL).
#pragma once
#include <cstdint>

#include "layout.hpp"

// how the kernels make a wave-uniform value provably uniform (readfirstlane); the identity everywhere else
#ifndef PT_CAM_UNIFORM
#define PT_CAM_UNIFORM(v) (v)
#endif

namespace pt {

constexpr float CAM_MARGIN_PIX = 0.125f;
constexpr float CAM_SLACK_REL = 1.0f / (float)(1u << 20);
constexpr uint32_t CAM_LIST_CAP = 16u;                 // triangle indices a work item keeps (64 B of LDS: what the 16-wave kernels have left)
constexpr uint32_t CAM_WALK_STACK = 96u;               // links the walk may have pending: <= 3 per level of a tree of < STACK_DEPTH levels

// outward normals of the five planes (left-to-right: x high, x low, y high, y low side, behind the apex) and |n|_1 of each
struct CamPyramid { float n[5][3]; float n1[5]; };

PT_HD inline float cam_abs(float v) { return v < 0.0f ? -v : v; }
PT_HD inline float cam_min(float a, float b) { return a < b ? a : b; }
PT_HD inline float cam_max(float a, float b) { return a < b ? b : a; }

// the pyramid of the pixels [x0, x1] x [y0, y1] (inclusive; x0 <= x1 < width, y0 <= y1 < height need not hold: a rectangle that sticks out
// of the frame only makes the pyramid larger)
PT_HD inline CamPyramid cam_pyramid(const DevCamera& cam, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    // regen_path: fx in [px, px + 1], dx = (2 fx / W - 1) * aspect * tan, dy = (1 - 2 fy / H) * tan (dy falls as y grows)
    const float fx_lo = (float)x0 - CAM_MARGIN_PIX, fx_hi = (float)x1 + 1.0f + CAM_MARGIN_PIX;
    const float fy_lo = (float)y0 - CAM_MARGIN_PIX, fy_hi = (float)y1 + 1.0f + CAM_MARGIN_PIX;
    const float dx_lo = (2.0f * fx_lo / (float)cam.width - 1.0f) * cam.aspect * cam.tan_half_fov;
    const float dx_hi = (2.0f * fx_hi / (float)cam.width - 1.0f) * cam.aspect * cam.tan_half_fov;
    const float dy_hi = (1.0f - 2.0f * fy_lo / (float)cam.height) * cam.tan_half_fov;
    const float dy_lo = (1.0f - 2.0f * fy_hi / (float)cam.height) * cam.tan_half_fov;
    // a point P = (s dx + u dy + f) * tau, tau > 0, has P.s = dx (P.f), P.u = dy (P.f), P.f > 0: inside means (s - dx_hi f) . P <= 0, ...
    CamPyramid py;
    for (int a = 0; a < 3; ++a) {
        py.n[0][a] = cam.s[a] - dx_hi * cam.f[a];
        py.n[1][a] = dx_lo * cam.f[a] - cam.s[a];
        py.n[2][a] = cam.u[a] - dy_hi * cam.f[a];
        py.n[3][a] = dy_lo * cam.f[a] - cam.u[a];
        py.n[4][a] = -cam.f[a];
    }
    for (int k = 0; k < 5; ++k) py.n1[k] = cam_abs(py.n[k][0]) + cam_abs(py.n[k][1]) + cam_abs(py.n[k][2]);
    return py;
}

// is the box [lo, hi] wholly outside one of the pyramid's planes?  extent: R of the error bound above
PT_HD inline bool cam_box_outside(const CamPyramid& py, const float lo[3], const float hi[3], float extent) {
    bool outside = false;
    for (int k = 0; k < 5; ++k) {
        const float m = cam_min(py.n[k][0] * lo[0], py.n[k][0] * hi[0]) + cam_min(py.n[k][1] * lo[1], py.n[k][1] * hi[1]) +
                        cam_min(py.n[k][2] * lo[2], py.n[k][2] * hi[2]);
        outside = outside || m > CAM_SLACK_REL * py.n1[k] * extent;
    }
    return outside;
}

// a slot of a DevNode4 that holds a child (unused slots: a point box at +FLT_MAX, bvh_builder.cpp collapse_bvh4)
PT_HD inline bool cam_slot_used(const DevNode4& nd, int c) { return nd.lox[c] <= nd.hix[c] && nd.lox[c] < 3.402823466e+38f; }

// R: the largest coordinate magnitude of the root's child boxes (every box of the tree lies inside their union)
PT_HD inline float cam_tree_extent(const DevNode4* nodes, int32_t root4) {
    float r = 0.0f;
    if (root4 < 0) return r;
    const DevNode4& nd = nodes[root4];
    for (int c = 0; c < 4; ++c) {
        if (!cam_slot_used(nd, c)) continue;
        r = cam_max(r, cam_max(cam_max(cam_abs(nd.lox[c]), cam_abs(nd.hix[c])), cam_max(cam_abs(nd.loy[c]), cam_abs(nd.hiy[c]))));
        r = cam_max(r, cam_max(cam_abs(nd.loz[c]), cam_abs(nd.hiz[c])));
    }
    return r;
}

struct CamWalk { uint32_t count; bool overflow; };     // count <= cap entries of `out` are valid; overflow: the list is NOT complete

// Walks the 4-wide tree from root4 and writes to out[0 .. count) the index of every triangle that lies in a leaf whose box is not outside
// the pyramid and whose OWN bounds are not outside it either (a leaf holds up to MAX_LEAF_TRIS triangles: their common box is larger than
// each).  tris / tri_shift: DevScene::tris and DevScene::tri_shift, the vertices the traversal's triangle test reads — render-space
// vertices are those minus tri_shift (tri_origin adds it to the ray's origin), one more rounding of at most u (R + |tri_shift|), which is
// why the triangle's bounds are tested with R + max |tri_shift| as the extent: 4 u |n|_1 of that against a slack of 16 u.
// overflow: more than `cap` triangles, or more than CAM_WALK_STACK links pending (no tree the builder makes) — the caller then traverses
// as if there were no list.  `stack`: CAM_WALK_STACK words of scratch (the kernels: LDS).  Every value the walk branches on is a function
// of its arguments alone: a wave whose lanes all call it with the same arguments runs it uniformly.
PT_HD inline CamWalk cam_walk(const DevNode4* nodes, int32_t root4, const DevTri* tris, const float tri_shift[3], const CamPyramid& py, uint32_t* out,
                              uint32_t cap, uint32_t* stack) {
    CamWalk w{0u, false};
    const float extent = cam_tree_extent(nodes, root4);
    const float extent_tri = extent + cam_max(cam_max(cam_abs(tri_shift[0]), cam_abs(tri_shift[1])), cam_abs(tri_shift[2]));
    uint32_t sp = 0u;
    int32_t cur = root4;
    for (;;) {
        // (every record is read WHOLE before anything is decided on it: the kernels' walk is a chain of dependent fetches, and a load
        // behind a branch on the previous load's value is one more round trip — the node's eight quads, a leaf's triangles, go out together)
        if (cur < 0) {
            const uint32_t first = leaf_first(cur), cnt = leaf_count(cur);
            for (uint32_t base = 0; base < cnt; base += 4u) {
                DevTri t[4];
                for (uint32_t i = 0; i < 4u; ++i) t[i] = tris[first + (base + i < cnt ? base + i : cnt - 1u)];      // (past the leaf's end: its last triangle again)
                bool keep[4];
                for (uint32_t i = 0; i < 4u; ++i) {
                    const float v[3][3] = {{t[i].p0[0], t[i].p0[1], t[i].p0[2]}, {t[i].p1x, t[i].p1yz[0], t[i].p1yz[1]}, {t[i].p2xy[0], t[i].p2xy[1], t[i].p2z}};
                    float lo[3], hi[3];
                    for (int a = 0; a < 3; ++a) {
                        lo[a] = cam_min(cam_min(v[0][a], v[1][a]), v[2][a]) - tri_shift[a];
                        hi[a] = cam_max(cam_max(v[0][a], v[1][a]), v[2][a]) - tri_shift[a];
                    }
                    keep[i] = base + i < cnt && !cam_box_outside(py, lo, hi, extent_tri);
                }
                for (uint32_t i = 0; i < 4u; ++i) {
                    if (!keep[i]) continue;
                    if (w.count >= cap) { w.overflow = true; return w; }
                    out[w.count++] = first + base + i;
                }
            }
        } else {
            const DevNode4 nd = nodes[cur];
            bool keep[4];
            for (int c = 0; c < 4; ++c) {
                const float lo[3] = {nd.lox[c], nd.loy[c], nd.loz[c]}, hi[3] = {nd.hix[c], nd.hiy[c], nd.hiz[c]};
                keep[c] = cam_slot_used(nd, c) && !cam_box_outside(py, lo, hi, extent);     // (an unused slot's planes are +FLT_MAX: whatever the products give, it is not kept)
            }
            for (int c = 0; c < 4; ++c) {
                if (!keep[c]) continue;
                if (sp >= CAM_WALK_STACK) { w.overflow = true; return w; }
                stack[sp++] = (uint32_t)nd.child[c];
            }
        }
        if (sp == 0u) return w;
        cur = (int32_t)PT_CAM_UNIFORM(stack[--sp]);
    }
}

}  // namespace pt
