// Moving the camera of a built scene (include/mi355pt_rebase.h): what does not need a device.  Pure — no HIP header, no environment, no
// clock — like launch_plan.hpp; tests/rebase_plan_check.cpp includes it alone.  Three things live here:
//
//   1. THE min / max of the refit.  A box plane is the exact min / max of vertex coordinates, so it does not depend on the order of the
//      reduction — except for the sign of a zero: -0.0 == +0.0 compares equal and a min has to pick one.  Both host builders pick with
//      std::min / std::max and glibc's fmin / fmax, all of which keep their FIRST operand when the two compare equal.  rb_min / rb_max are
//      that expression, written as one compare and one select so that the device cannot turn it into v_min_f32 (which orders -0 < +0);
//      host refit (mi355pt_scene_debug_move_digest) and device refit (pt_kernels_rebase.hip) both call the functions below.
//   2. The refit of one BVH2 child box and the pad of one 4-wide slot, as PT_HD functions.
//   3. The plan: the BVH2's (node, side) pairs grouped by the node's height, and for every used slot of the 4-wide tree the BVH2
//      (node, side) whose box it carries.  Derived from the links alone.
#pragma once
#include <cfloat>
#include <cstdint>
#include <vector>

#include "layout.hpp"

namespace pt {

PT_HD inline float rb_min(float a, float b) { return b < a ? b : a; }
PT_HD inline float rb_max(float a, float b) { return a < b ? b : a; }
PT_HD inline float rb_abs(float v) { return v < 0.0f ? -v : v; }

// the 9 position floats of a DevTri, vertex v, axis a
PT_HD inline float tri_coord(const DevTri& t, int v, int a) {
    return v == 0 ? t.p0[a] : v == 1 ? (a == 0 ? t.p1x : t.p1yz[a - 1]) : (a == 2 ? t.p2z : t.p2xy[a]);
}

// Stage A's BuildTri bounds (scene_lower.cpp lower_triangles): fmin(v0, fmin(v1, v2))
PT_HD inline void tri_bounds(const DevTri& t, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) {
        const float v0 = tri_coord(t, 0, a), v1 = tri_coord(t, 1, a), v2 = tri_coord(t, 2, a);
        lo[a] = rb_min(v0, rb_min(v1, v2)); hi[a] = rb_max(v0, rb_max(v1, v2));
    }
}

// BVH2 child `side` of a node: is it there?  (the wrapped single-leaf root's second child is a point box at +FLT_MAX: bvh_builder.cpp)
PT_HD inline bool child_used(const DevNode& n, int side) { return n.bx[side] <= n.bx[2 + side] && n.bx[side] < FLT_MAX; }

// The box of the child behind `link`: a leaf's from its triangles in leaf order (Box::grow from +-FLT_MAX), a node's as the union of that
// node's two child boxes, first child first.  `nodes` must already hold the refit boxes of every node below.
PT_HD inline void refit_child_box(const DevNode* nodes, const DevTri* tris, int32_t link, float lo[3], float hi[3]) {
    if (link < 0) {
        const uint32_t first = leaf_first(link), count = leaf_count(link);
        for (int a = 0; a < 3; ++a) { lo[a] = FLT_MAX; hi[a] = -FLT_MAX; }
        for (uint32_t k = 0; k < count; ++k) {
            float tl[3], th[3];
            tri_bounds(tris[first + k], tl, th);
            for (int a = 0; a < 3; ++a) { lo[a] = rb_min(lo[a], tl[a]); hi[a] = rb_max(hi[a], th[a]); }
        }
    } else {
        const DevNode& n = nodes[link];
        lo[0] = rb_min(n.bx[0], n.bx[1]); hi[0] = rb_max(n.bx[2], n.bx[3]);
        lo[1] = rb_min(n.by[0], n.by[1]); hi[1] = rb_max(n.by[2], n.by[3]);
        lo[2] = rb_min(n.bz[0], n.bz[1]); hi[2] = rb_max(n.bz[2], n.bz[3]);
    }
}
PT_HD inline void store_child_box(DevNode& n, int side, const float lo[3], const float hi[3]) {
    n.bx[side] = lo[0]; n.bx[2 + side] = hi[0]; n.by[side] = lo[1]; n.by[2 + side] = hi[1]; n.bz[side] = lo[2]; n.bz[2 + side] = hi[2];
}

// pad_nodes4's r (scene_lower.cpp): the largest coordinate magnitude over the used slots of the 4-wide tree.  Every slot carries a BVH2
// child box, every such box lies inside one of the root's two child boxes, and those are exact extremes of vertex coordinates, which a
// deeper box attains: the largest magnitude over the root record's used children IS r (tests/rebase_plan_check.cpp, tests/test_rebase.py).
PT_HD inline float pad_radius(const DevNode& root) {
    float r = 0.0f;
    for (int side = 0; side < 2; ++side) {
        if (!child_used(root, side)) continue;
        const float v[6] = {root.bx[side], root.by[side], root.bz[side], root.bx[2 + side], root.by[2 + side], root.bz[2 + side]};
        for (int k = 0; k < 6; ++k) r = rb_max(r, rb_abs(v[k]));
    }
    return r;
}
// one used slot of a DevNode4 takes the box of BVH2 (node, side) `src`, padded like pad_nodes4 pads it (pad = 0 without PT_NODE_FMA)
PT_HD inline void store_slot_box(DevNode4& d, int c, const DevNode& s, int side, float pad) {
    d.lox[c] = s.bx[side] - pad; d.loy[c] = s.by[side] - pad; d.loz[c] = s.bz[side] - pad;
    d.hix[c] = s.bx[2 + side] + pad; d.hiy[c] = s.by[2 + side] + pad; d.hiz[c] = s.bz[2 + side] + pad;
}
PT_HD inline bool slot4_used(const DevNode4& n, int c) { return n.lox[c] <= n.hix[c] && n.lox[c] < FLT_MAX; }

constexpr uint32_t REBASE_NO_SOURCE = 0xffffffffu;

// entry = node << 1 | side
struct RebasePlan {
    std::vector<uint32_t> entries;         // the used (node, side) pairs of the nodes reachable from the root, grouped by the node's height
    std::vector<uint32_t> height_offset;   // group h (height h + 1) is entries[height_offset[h] .. height_offset[h + 1]); size = heights + 1
    std::vector<uint32_t> node_height;     // per node; 0: not reachable
    std::vector<uint32_t> slot_src;        // 4 per DevNode4: the entry whose box the slot carries, REBASE_NO_SOURCE for an unused slot
    uint32_t heights() const { return height_offset.empty() ? 0u : (uint32_t)height_offset.size() - 1u; }
};

// false: the two trees are not a BVH2 and its collapse (a link out of range, a height above MAX_BUILD_DEPTH + 1, a slot without a source)
inline bool make_rebase_plan(const std::vector<DevNode>& nodes, int32_t root, const std::vector<DevNode4>& nodes4, int32_t root4, size_t n_tris, RebasePlan* plan) {
    *plan = RebasePlan{};
    plan->slot_src.assign(nodes4.size() * 4, REBASE_NO_SOURCE);
    if (root < 0 || nodes.empty()) return nodes4.empty();           // the root is a leaf: nothing to refit
    if ((size_t)root >= nodes.size()) return false;
    const size_t n = nodes.size();
    // heights, children first: height 1 = both children are leaves, otherwise 1 + the larger child height
    std::vector<int32_t> order; order.reserve(n);
    std::vector<int32_t> st{root};
    std::vector<uint32_t> parent(n, REBASE_NO_SOURCE);              // the entry that links to the node
    std::vector<uint32_t> leaf_entry(n_tris, REBASE_NO_SOURCE);     // by leaf_first: the entry that links to the leaf
    while (!st.empty()) {
        const int32_t v = st.back(); st.pop_back();
        if (order.size() >= n) return false;                        // a cycle or a shared child
        order.push_back(v);
        for (int c = 0; c < 2; ++c) {
            if (!child_used(nodes[(size_t)v], c)) continue;
            const int32_t l = nodes[(size_t)v].child[c];
            const uint32_t e = ((uint32_t)v << 1) | (uint32_t)c;
            if (l >= 0) { if ((size_t)l >= n || parent[(size_t)l] != REBASE_NO_SOURCE || l == root) return false; parent[(size_t)l] = e; st.push_back(l); }
            else { if ((size_t)leaf_first(l) + leaf_count(l) > n_tris || leaf_entry[leaf_first(l)] != REBASE_NO_SOURCE) return false; leaf_entry[leaf_first(l)] = e; }
        }
    }
    plan->node_height.assign(n, 0u);
    uint32_t top = 0;
    for (size_t q = order.size(); q-- > 0;) {
        const DevNode& nd = nodes[(size_t)order[q]];
        uint32_t h = 1;
        for (int c = 0; c < 2; ++c) if (child_used(nd, c) && nd.child[c] >= 0) h = h > 1u + plan->node_height[(size_t)nd.child[c]] ? h : 1u + plan->node_height[(size_t)nd.child[c]];
        plan->node_height[(size_t)order[q]] = h;
        top = top > h ? top : h;
    }
    if (top > (uint32_t)MAX_BUILD_DEPTH + 1u) return false;
    plan->height_offset.assign((size_t)top + 1, 0u);
    for (int32_t v : order) for (int c = 0; c < 2; ++c) if (child_used(nodes[(size_t)v], c)) ++plan->height_offset[plan->node_height[(size_t)v]];
    {   // counts at [h] for height h -> offsets: group h - 1 starts at the sum of the counts below
        uint32_t sum = 0;
        std::vector<uint32_t> begin((size_t)top + 1, 0u);
        for (uint32_t h = 1; h <= top; ++h) { begin[h - 1] = sum; sum += plan->height_offset[h]; }
        begin[top] = sum;
        plan->height_offset = begin;
    }
    plan->entries.assign(plan->height_offset[top], 0u);
    {
        std::vector<uint32_t> next(plan->height_offset.begin(), plan->height_offset.end() - 1);
        for (size_t v = 0; v < n; ++v) {                             // ascending node index inside a group
            const uint32_t h = plan->node_height[v];
            if (!h) continue;
            for (int c = 0; c < 2; ++c) if (child_used(nodes[v], c)) plan->entries[next[h - 1]++] = ((uint32_t)v << 1) | (uint32_t)c;
        }
    }
    // the 4-wide tree: a node's used slots are a cut through the subtree of ONE BVH2 node.  A leaf slot's source is the entry that links to
    // that leaf; an inner slot's source is the entry that links to the BVH2 node its child stands for; and the BVH2 node a 4-wide node
    // stands for is the one node among its slots' sources whose own parent is not among them.
    if (root4 < 0 || (size_t)root4 >= nodes4.size()) return false;
    std::vector<int32_t> stands_for(nodes4.size(), -1);
    std::vector<int32_t> post; post.reserve(nodes4.size());
    std::vector<int32_t> st4{root4};
    while (!st4.empty()) {
        const int32_t v = st4.back(); st4.pop_back();
        if (post.size() >= nodes4.size()) return false;
        post.push_back(v);
        for (int c = 0; c < 4; ++c) if (slot4_used(nodes4[(size_t)v], c) && nodes4[(size_t)v].child[c] >= 0) {
            if ((size_t)nodes4[(size_t)v].child[c] >= nodes4.size()) return false;
            st4.push_back(nodes4[(size_t)v].child[c]);
        }
    }
    for (size_t q = post.size(); q-- > 0;) {
        const size_t v = (size_t)post[q];
        const DevNode4& nd = nodes4[v];
        uint32_t src[4]; int k = 0;
        for (int c = 0; c < 4; ++c) {
            if (!slot4_used(nd, c)) continue;
            const int32_t l = nd.child[c];
            uint32_t e;
            if (l < 0) { if (leaf_first(l) >= n_tris) return false; e = leaf_entry[leaf_first(l)]; }
            else { if (stands_for[(size_t)l] < 0) return false; e = (int32_t)stands_for[(size_t)l] == root ? REBASE_NO_SOURCE : parent[(size_t)stands_for[(size_t)l]]; }
            if (e == REBASE_NO_SOURCE) return false;
            plan->slot_src[4 * v + (size_t)c] = e;
            src[k++] = e;
        }
        if (k == 0) return false;
        // the nodes among the sources whose parent is not: one — that is the node; two — both children of the node were opened (a, b
        // under v give the slots a0 a1 b0 b1) and the node is their common parent
        int32_t top[2] = {-1, -1}; int n_top = 0;
        for (int i = 0; i < k; ++i) {
            const int32_t node = (int32_t)(src[i] >> 1);
            const uint32_t up = node == root ? REBASE_NO_SOURCE : parent[(size_t)node];
            bool inside = false;
            for (int j = 0; j < k; ++j) if (up != REBASE_NO_SOURCE && (src[j] >> 1) == (up >> 1)) inside = true;
            if (inside || (n_top > 0 && top[0] == node) || (n_top > 1 && top[1] == node)) continue;
            if (n_top == 2) return false;
            top[n_top++] = node;
        }
        if (n_top == 1) stands_for[v] = top[0];
        else if (n_top == 2 && top[0] != root && top[1] != root && (parent[(size_t)top[0]] >> 1) == (parent[(size_t)top[1]] >> 1)) stands_for[v] = (int32_t)(parent[(size_t)top[0]] >> 1);
        else return false;
    }
    return stands_for[(size_t)root4] == root;
}

// The host form of the three kernels' tree work: every box of the BVH2 from `tris` (leaf order, render space), lowest height first, then
// every used slot of the 4-wide tree from its source, padded.  What mi355pt_scene_debug_move_digest hashes.
inline void refit_host(const RebasePlan& plan, int32_t root, const DevTri* tris, std::vector<DevNode>* nodes, std::vector<DevNode4>* nodes4) {
    for (uint32_t e : plan.entries) {                               // already lowest height first
        DevNode& nd = (*nodes)[e >> 1];
        float lo[3], hi[3];
        refit_child_box(nodes->data(), tris, nd.child[e & 1u], lo, hi);
        store_child_box(nd, (int)(e & 1u), lo, hi);
    }
    if (root < 0 || nodes->empty()) return;
#if PT_NODE_FMA
    const float pad = pad_radius((*nodes)[(size_t)root]) * NODE4_PAD_REL;
#else
    const float pad = 0.0f;
#endif
    for (size_t i = 0; i < plan.slot_src.size(); ++i) {
        const uint32_t e = plan.slot_src[i];
        if (e != REBASE_NO_SOURCE) store_slot_box((*nodes4)[i >> 2], (int)(i & 3u), (*nodes)[e >> 1], (int)(e & 1u), pad);
    }
}

}  // namespace pt
