// TEST INFRASTRUCTURE ONLY.  csrc/rebase_plan.hpp on its own (plain g++, no HIP): seeded BVH2 trees of random triangles (object-median
// splits at random positions, leaves of 1 .. MAX_LEAF_TRIS), a random collapse to the 4-wide layout (each node's two children opened at
// random until four slots are used or none can be opened), and for each pair
//   - the height groups partition the used (node, side) pairs, a node's height is 1 + the larger child height, every child node of a
//     group lies in a lower group;
//   - the slot map names a source for exactly the used slots, and the source's box IS the slot's box;
//   - after the triangles move, refit_host gives every BVH2 child the exact min / max of the vertices below it, every used slot its
//     source's box moved out by the pad, unused slots untouched; pad_radius(root record) equals the loop over the used slots' boxes;
// then the shapes the builders make at the edges: a root that is a leaf (no node), the wrapped single leaf (one node, second child a
// point box at +FLT_MAX), a one-node tree of two leaves; and rb_min / rb_max keep their first operand when -0.0 meets +0.0.
// usage: rebase_plan_check <seed> <n_tris>   ->   "ok <nodes> <nodes4> <heights> <entries>"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "rebase_plan.hpp"

using namespace pt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {

std::mt19937 rng;
float uni(float a, float b) { return a + (b - a) * (float)(rng() >> 8) * (1.0f / 16777216.0f); }

void set_tri(DevTri& t, const float v[9]) {
    t.p0[0] = v[0]; t.p0[1] = v[1]; t.p0[2] = v[2]; t.p1x = v[3]; t.p1yz[0] = v[4]; t.p1yz[1] = v[5]; t.p2xy[0] = v[6]; t.p2xy[1] = v[7]; t.p2z = v[8];
    t.instance = 0; t.flags = 1; t.mclass = 0;
}
void exact_box(const std::vector<DevTri>& tris, uint32_t first, uint32_t count, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t k = first; k < first + count; ++k) for (int v = 0; v < 3; ++v) for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], tri_coord(tris[k], v, a)); hi[a] = std::max(hi[a], tri_coord(tris[k], v, a));
    }
}

struct Tree {
    std::vector<DevTri> tris;
    std::vector<DevNode> nodes;
    std::vector<DevNode4> nodes4;
    int32_t root = 0, root4 = 0;
    // leaf-ordered triangles [first, first + count) -> link; fills lo / hi with the exact box
    int32_t build(uint32_t first, uint32_t count, float lo[3], float hi[3], bool may_leaf = true) {
        exact_box(tris, first, count, lo, hi);
        if (may_leaf && count <= (uint32_t)MAX_LEAF_TRIS && (count == 1 || rng() % 3 == 0)) return make_leaf(first, count);
        const uint32_t left = std::min(count - 1, std::max(1u, count / 3 + (uint32_t)(rng() % (count - 2 * (count / 3)))));   // depth <= log1.5(n)
        const size_t me = nodes.size();
        nodes.emplace_back();
        float l0[3], h0[3], l1[3], h1[3];
        const int32_t c0 = build(first, left, l0, h0), c1 = build(first + left, count - left, l1, h1);
        DevNode& nd = nodes[me];
        std::memset(&nd, 0, sizeof(nd));
        store_child_box(nd, 0, l0, h0); store_child_box(nd, 1, l1, h1);
        nd.child[0] = c0; nd.child[1] = c1;
        return (int32_t)me;
    }
    struct Member { int32_t node; int side; };
    int32_t collapse(int32_t link) {
        if (link < 0) return link;
        std::vector<Member> m = {{link, 0}, {link, 1}};
        if (!child_used(nodes[(size_t)link], 1)) m.pop_back();
        while (m.size() < 4) {
            std::vector<size_t> open;
            for (size_t i = 0; i < m.size(); ++i) if (nodes[(size_t)m[i].node].child[m[i].side] >= 0) open.push_back(i);
            if (open.empty() || rng() % 4 == 0) break;
            const size_t i = open[rng() % open.size()];
            const int32_t inner = nodes[(size_t)m[i].node].child[m[i].side];
            m[i] = {inner, 0}; m.push_back({inner, 1});
        }
        std::shuffle(m.begin(), m.end(), rng);
        const size_t me = nodes4.size();
        nodes4.emplace_back();
        int32_t links[4] = {0, 0, 0, 0};
        for (size_t c = 0; c < m.size(); ++c) links[c] = collapse(nodes[(size_t)m[c].node].child[m[c].side]);
        DevNode4& d = nodes4[me];
        std::memset(&d, 0, sizeof(d));
        for (int c = 0; c < 4; ++c) {
            if ((size_t)c < m.size()) { store_slot_box(d, c, nodes[(size_t)m[(size_t)c].node], m[(size_t)c].side, 0.0f); d.child[c] = links[c]; }
            else { d.lox[c] = d.loy[c] = d.loz[c] = d.hix[c] = d.hiy[c] = d.hiz[c] = FLT_MAX; }
        }
        return (int32_t)me;
    }
};

// the exact box below a link, from the triangles
void box_below(const Tree& t, int32_t link, float lo[3], float hi[3]) {
    if (link < 0) { exact_box(t.tris, leaf_first(link), leaf_count(link), lo, hi); return; }
    float l[2][3], h[2][3];
    for (int c = 0; c < 2; ++c) box_below(t, t.nodes[(size_t)link].child[c], l[c], h[c]);
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(l[0][a], l[1][a]); hi[a] = std::max(h[0][a], h[1][a]); }
}

int check_tree(Tree& t, const RebasePlan& plan) {
    const size_t n = t.nodes.size();
    // groups: every used side of every node once, in the group of its node's height
    std::vector<int> seen(2 * n, 0);
    CHECK(plan.height_offset.size() >= 2 && plan.height_offset[0] == 0 && plan.height_offset.back() == plan.entries.size());
    for (uint32_t h = 0; h < plan.heights(); ++h) {
        CHECK(plan.height_offset[h] < plan.height_offset[h + 1]);                 // no empty height
        for (uint32_t k = plan.height_offset[h]; k < plan.height_offset[h + 1]; ++k) {
            const uint32_t e = plan.entries[k];
            CHECK((e >> 1) < n && child_used(t.nodes[e >> 1], (int)(e & 1u)));
            CHECK(plan.node_height[e >> 1] == h + 1);
            ++seen[e];
            const int32_t l = t.nodes[e >> 1].child[e & 1u];
            if (l >= 0) CHECK(plan.node_height[(size_t)l] >= 1 && plan.node_height[(size_t)l] <= h);   // written by an earlier launch
        }
    }
    for (size_t v = 0; v < n; ++v) {
        uint32_t want = 1;
        for (int c = 0; c < 2; ++c) {
            CHECK(seen[2 * v + (size_t)c] == (child_used(t.nodes[v], c) ? 1 : 0));
            if (child_used(t.nodes[v], c) && t.nodes[v].child[c] >= 0) want = std::max(want, 1u + plan.node_height[(size_t)t.nodes[v].child[c]]);
        }
        CHECK(plan.node_height[v] == want);
    }
    CHECK(plan.heights() <= (uint32_t)MAX_BUILD_DEPTH + 1u);
    // the slot map: exactly the used slots, and the source's box is the slot's
    CHECK(plan.slot_src.size() == 4 * t.nodes4.size());
    for (size_t i = 0; i < plan.slot_src.size(); ++i) {
        const DevNode4& d = t.nodes4[i >> 2]; const int c = (int)(i & 3u);
        CHECK((plan.slot_src[i] != REBASE_NO_SOURCE) == slot4_used(d, c));
        if (plan.slot_src[i] == REBASE_NO_SOURCE) continue;
        const DevNode& s = t.nodes[plan.slot_src[i] >> 1]; const int side = (int)(plan.slot_src[i] & 1u);
        CHECK(child_used(s, side));
        if (s.child[side] < 0) CHECK(d.child[c] == s.child[side]);
        else CHECK(d.child[c] >= 0);
        DevNode4 want = d;
        store_slot_box(want, c, s, side, 0.0f);
        CHECK(std::memcmp(&want, &d, sizeof(d)) == 0);
    }
    // move the triangles (a translation, rounded per coordinate), refit, compare with the exact boxes
    const float shift[3] = {uni(-50.0f, 50.0f), uni(-5.0f, 5.0f), 0.0f};
    for (DevTri& tr : t.tris) {
        float v[9];
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) v[3 * k + a] = tri_coord(tr, k, a) + shift[a];
        set_tri(tr, v);
    }
    const std::vector<DevNode4> before4 = t.nodes4;
    refit_host(plan, t.root, t.tris.data(), &t.nodes, &t.nodes4);
    for (size_t v = 0; v < n; ++v) for (int c = 0; c < 2; ++c) {
        if (!child_used(t.nodes[v], c)) continue;
        float lo[3], hi[3];
        box_below(t, t.nodes[v].child[c], lo, hi);
        const DevNode& nd = t.nodes[v];                                           // as values: which zero a min keeps depends on the order
        CHECK(nd.bx[c] == lo[0] && nd.by[c] == lo[1] && nd.bz[c] == lo[2] && nd.bx[2 + c] == hi[0] && nd.by[2 + c] == hi[1] && nd.bz[2 + c] == hi[2]);
    }
    float r = 0.0f;                                                               // pad_nodes4's loop, over the boxes the slots carry
    for (size_t i = 0; i < plan.slot_src.size(); ++i) if (plan.slot_src[i] != REBASE_NO_SOURCE) {
        const DevNode& s = t.nodes[plan.slot_src[i] >> 1]; const int side = (int)(plan.slot_src[i] & 1u);
        for (float v : {s.bx[side], s.by[side], s.bz[side], s.bx[2 + side], s.by[2 + side], s.bz[2 + side]}) r = std::max(r, std::fabs(v));
    }
    CHECK(r == pad_radius(t.nodes[(size_t)t.root]));
#if PT_NODE_FMA
    const float pad = r * NODE4_PAD_REL;
#else
    const float pad = 0.0f;
#endif
    for (size_t i = 0; i < plan.slot_src.size(); ++i) {
        DevNode4 want = before4[i >> 2];
        for (int c = 0; c < 4; ++c) {
            const uint32_t e = plan.slot_src[4 * (i >> 2) + (size_t)c];
            if (e != REBASE_NO_SOURCE) store_slot_box(want, c, t.nodes[e >> 1], (int)(e & 1u), pad);
        }
        CHECK(std::memcmp(&want, &t.nodes4[i >> 2], sizeof(DevNode4)) == 0);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    const uint32_t n_tris = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 100u;
    rng.seed(seed);
    {   // the zero both sides pick
        const float nz = -0.0f, pz = 0.0f;
        CHECK(std::signbit(rb_min(nz, pz)) && !std::signbit(rb_min(pz, nz)) && std::signbit(rb_max(nz, pz)) && !std::signbit(rb_max(pz, nz)));
        CHECK(std::signbit(std::min(nz, pz)) && !std::signbit(std::min(pz, nz)) && std::signbit(std::max(nz, pz)) && !std::signbit(std::max(pz, nz)));
    }
    Tree t;
    t.tris.resize(n_tris);
    for (DevTri& tr : t.tris) {
        float v[9];
        const float c[3] = {uni(-1.0f, 1.0f), uni(-1.0f, 1.0f), uni(-4.0f, -2.0f)};
        for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + uni(-0.2f, 0.2f);
        if (rng() % 8 == 0) v[0] = v[3] = 0.0f;                                    // vertices on the plane x = 0, of both signs of zero
        if (rng() % 8 == 0) v[6] = -0.0f;
        set_tri(tr, v);
    }
    float lo[3], hi[3];
    RebasePlan plan;
    if (n_tris == 0) {                                                            // the edge shapes
        // a root that is a leaf: nothing to refit
        CHECK(make_rebase_plan({}, make_leaf(0, 3), {}, 0, 3, &plan) && plan.entries.empty() && plan.heights() == 0 && plan.slot_src.empty());
        // the wrapped single leaf: one node, both links the leaf, the second child a point box at +FLT_MAX (bvh_builder.cpp)
        Tree w;
        w.tris.resize(3);
        for (DevTri& tr : w.tris) { const float v[9] = {uni(-1, 1), uni(-1, 1), -3, uni(-1, 1), uni(-1, 1), -3, uni(-1, 1), uni(-1, 1), -2}; set_tri(tr, v); }
        exact_box(w.tris, 0, 3, lo, hi);
        w.nodes.emplace_back(); std::memset(&w.nodes[0], 0, sizeof(DevNode));
        store_child_box(w.nodes[0], 0, lo, hi);
        const float far_lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
        store_child_box(w.nodes[0], 1, far_lo, far_lo);
        w.nodes[0].child[0] = w.nodes[0].child[1] = make_leaf(0, 3);
        w.root = 0; w.root4 = w.collapse(0);
        CHECK(make_rebase_plan(w.nodes, w.root, w.nodes4, w.root4, 3, &plan));
        CHECK(plan.entries.size() == 1 && plan.entries[0] == 0u && plan.heights() == 1);
        CHECK(plan.slot_src[0] == 0u && plan.slot_src[1] == REBASE_NO_SOURCE && plan.slot_src[2] == REBASE_NO_SOURCE && plan.slot_src[3] == REBASE_NO_SOURCE);
        if (check_tree(w, plan)) return 1;
        CHECK(w.nodes[0].bx[1] == FLT_MAX && w.nodes[0].bz[3] == FLT_MAX);          // the empty child stays
        // a one-node tree of two leaves
        Tree o;
        o.tris = w.tris;
        o.nodes.emplace_back(); std::memset(&o.nodes[0], 0, sizeof(DevNode));
        exact_box(o.tris, 0, 2, lo, hi); store_child_box(o.nodes[0], 0, lo, hi);
        exact_box(o.tris, 2, 1, lo, hi); store_child_box(o.nodes[0], 1, lo, hi);
        o.nodes[0].child[0] = make_leaf(0, 2); o.nodes[0].child[1] = make_leaf(2, 1);
        o.root = 0; o.root4 = o.collapse(0);
        CHECK(make_rebase_plan(o.nodes, o.root, o.nodes4, o.root4, 3, &plan));
        CHECK(plan.entries.size() == 2 && plan.heights() == 1);
        if (check_tree(o, plan)) return 1;
        // broken trees are refused, not walked: a link out of range, a child reached twice
        o.nodes[0].child[1] = 5;
        CHECK(!make_rebase_plan(o.nodes, o.root, o.nodes4, o.root4, 3, &plan));
        o.nodes[0].child[1] = make_leaf(0, 2);
        CHECK(!make_rebase_plan(o.nodes, o.root, o.nodes4, o.root4, 3, &plan));
        std::printf("ok 1 1 1 2\n");
        return 0;
    }
    t.root = t.build(0, n_tris, lo, hi, false);                                  // (n_tris >= 2: the root is a node)
    CHECK(t.root >= 0);
    t.root4 = t.collapse(t.root);
    CHECK(make_rebase_plan(t.nodes, t.root, t.nodes4, t.root4, n_tris, &plan));
    if (check_tree(t, plan)) return 1;
    std::printf("ok %zu %zu %u %zu\n", t.nodes.size(), t.nodes4.size(), plan.heights(), plan.entries.size());
    return 0;
}
