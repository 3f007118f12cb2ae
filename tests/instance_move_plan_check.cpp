// TEST INFRASTRUCTURE ONLY.  csrc/instance_move_plan.hpp on its own (plain g++, no HIP):
//   - shade_normal against the expression scene_lower.cpp lower_triangles held before the two shared it, restated here with std::sqrt and
//     its own vector type — bit for bit — and against a double-precision normal through the inverse-transpose (angle below 5e-5), on seeded
//     triangles under rotation, non-uniform scale and mirror matrices and under the identity class;
//   - half_area and the fixed-order sum against long double: n terms of random boxes and leaf counts, relative error within
//     (ceil(log2 n) + 3) 2^-24 — each value goes through at most ceil(log2 n) additions that round (the tree over zero-padded blocks adds
//     +0.0 exactly), all terms are positive so nothing cancels, and 3 ulps cover the rounding of a term itself;
//   - the block structure: the sum of n terms equals the sum of the block sums of SAH_BLOCK terms, for n around SAH_BLOCK and SAH_BLOCK^2;
//   - hand-made trees: two leaves whose cost is computed by hand, the single-leaf root (cost 0), the wrapped single leaf, a chain.
// usage: instance_move_plan_check <seed> <n>   ->   "ok <n>"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "instance_move_plan.hpp"

using namespace pt;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

namespace {

std::mt19937 rng;
float uni(float a, float b) { return a + (b - a) * (float)(rng() >> 8) * (1.0f / 16777216.0f); }

// the lowering's expression as scene_lower.cpp wrote it out (V3, cross, dot, length, normalize of that file)
struct V3 { float x, y, z; };
V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 cross(V3 a, V3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
float length(V3 a) { return std::sqrt(dot(a, a)); }
V3 normalize(V3 a) { float r = 1.0f / length(a); return {a.x * r, a.y * r, a.z * r}; }
V3 lowering_normal(const V3 pl[3], const float* inv, bool identity) {
    V3 n = normalize(normalize(cross(pl[1] - pl[0], pl[2] - pl[0])));
    if (!identity)
        n = V3{(inv[0] * n.x + inv[1] * n.y) + inv[2] * n.z, (inv[3] * n.x + inv[4] * n.y) + inv[5] * n.z, (inv[6] * n.x + inv[7] * n.y) + inv[8] * n.z};
    return normalize(n);
}

// a column-major 3x3 and its inverse in double
void inverse3(const double a[9], double inv[9]) {
    const double det = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2]) + a[6] * (a[1] * a[5] - a[4] * a[2]);
    const double r[9] = {(a[4] * a[8] - a[7] * a[5]) / det, -(a[1] * a[8] - a[7] * a[2]) / det, (a[1] * a[5] - a[4] * a[2]) / det,
                         -(a[3] * a[8] - a[6] * a[5]) / det, (a[0] * a[8] - a[6] * a[2]) / det, -(a[0] * a[5] - a[3] * a[2]) / det,
                         (a[3] * a[7] - a[6] * a[4]) / det, -(a[0] * a[7] - a[6] * a[1]) / det, (a[0] * a[4] - a[3] * a[1]) / det};
    for (int i = 0; i < 9; ++i) inv[i] = r[i];
}
// kind 0: rotation about a random axis; 1: rotation x non-uniform scale; 2: the same with one axis mirrored
void random_matrix(int kind, double m[9]) {
    double ax[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
    const double l = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-9;
    for (double& v : ax) v /= l;
    const double th = uni(-3.1f, 3.1f), c = std::cos(th), s = std::sin(th), t = 1 - c;
    const double rot[9] = {t * ax[0] * ax[0] + c, t * ax[0] * ax[1] + s * ax[2], t * ax[0] * ax[2] - s * ax[1],
                           t * ax[0] * ax[1] - s * ax[2], t * ax[1] * ax[1] + c, t * ax[1] * ax[2] + s * ax[0],
                           t * ax[0] * ax[2] + s * ax[1], t * ax[1] * ax[2] - s * ax[0], t * ax[2] * ax[2] + c};
    double sc[3] = {1, 1, 1};
    if (kind >= 1) for (double& v : sc) v = uni(0.2f, 5.0f);
    if (kind == 2) sc[rng() % 3] *= -1.0;
    for (int col = 0; col < 3; ++col) for (int r = 0; r < 3; ++r) m[3 * col + r] = (double)(float)(rot[3 * col + r] * sc[col]);
}

int check_normals(int count) {
    for (int i = 0; i < count; ++i) {
        const int kind = i % 4;                                       // 3: the identity class (inv is not read)
        double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, invd[9];
        if (kind < 3) random_matrix(kind, m);
        inverse3(m, invd);
        float inv[9];
        for (int k = 0; k < 9; ++k) inv[k] = (float)invd[k];
        V3 p[3];
        const float size = i % 3 == 0 ? 1e-3f : i % 3 == 1 ? 1.0f : 300.0f;
        for (V3& v : p) v = V3{uni(-size, size), uni(-size, size), uni(-size, size)};
        const V3 want = lowering_normal(p, inv, kind == 3);
        const IV3 got = shade_normal(IV3{p[0].x, p[0].y, p[0].z}, IV3{p[1].x, p[1].y, p[1].z}, IV3{p[2].x, p[2].y, p[2].z}, inv, kind == 3);
        CHECK(std::memcmp(&want, &got, 12) == 0);
        // the normal of the transformed triangle, in double: transpose(inverse) * n
        const double e1[3] = {(double)p[1].x - p[0].x, (double)p[1].y - p[0].y, (double)p[1].z - p[0].z}, e2[3] = {(double)p[2].x - p[0].x, (double)p[2].y - p[0].y, (double)p[2].z - p[0].z};
        const double n[3] = {e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0], e1[0] * e2[1] - e2[0] * e1[1]};
        double w[3];
        for (int r = 0; r < 3; ++r) w[r] = kind == 3 ? n[r] : invd[3 * r] * n[0] + invd[3 * r + 1] * n[1] + invd[3 * r + 2] * n[2];
        const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (wl > 0) {
            const double gl = std::sqrt((double)got.x * got.x + (double)got.y * got.y + (double)got.z * got.z);
            CHECK(std::fabs(gl - 1.0) < 1e-6);
            const double cosang = (w[0] * got.x + w[1] * got.y + w[2] * got.z) / (wl * gl);
            CHECK(cosang > 1.0 - 1e-9);                               // angle below 5e-5 rad
        }
    }
    return 0;
}

int ceil_log2(uint32_t n) { int k = 0; while ((1ull << k) < n) ++k; return k; }

int check_sums(uint32_t n) {
    std::vector<DevNode> nodes((n + 1) / 2);
    std::vector<uint32_t> entries;
    long double exact = 0.0L;
    for (uint32_t k = 0; k < n; ++k) {
        DevNode& nd = nodes[k >> 1];
        const int side = (int)(k & 1u);
        if (side == 0) std::memset(&nd, 0, sizeof(nd));
        float lo[3], hi[3];
        const float scale = k % 5 == 0 ? 1e-3f : k % 5 == 1 ? 100.0f : 1.0f;
        for (int a = 0; a < 3; ++a) { lo[a] = uni(-scale, scale); hi[a] = lo[a] + uni(0.0f, scale); }
        store_child_box(nd, side, lo, hi);
        const uint32_t count = 1u + rng() % (uint32_t)MAX_LEAF_TRIS;
        nd.child[side] = rng() % 2 ? make_leaf(k, count) : (int32_t)(k >> 1);
        entries.push_back(k);
        const long double dx = (long double)hi[0] - lo[0], dy = (long double)hi[1] - lo[1], dz = (long double)hi[2] - lo[2];
        const long double ha = (dx * dy + dy * dz) + dz * dx;
        CHECK(std::fabs((double)((long double)half_area(lo, hi) - ha)) <= (double)(3.0L * ha * 5.9604644775390625e-8L));
        exact += ha * (nd.child[side] < 0 ? (long double)count : 1.0L);
    }
    if (n & 1u) { float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}; store_child_box(nodes.back(), 1, lo, lo); }      // the last node's second child: unused
    std::vector<float> terms(n);
    for (uint32_t k = 0; k < n; ++k) terms[k] = sah_term(nodes[k >> 1], (int)(k & 1u));
    const float sum = sah_sum_host(terms);
    const long double bound = (long double)(ceil_log2(n) + 3) * 5.9604644775390625e-8L;
    CHECK(exact > 0.0L && std::fabs((double)(((long double)sum - exact) / exact)) <= (double)bound);
    // the block structure: block sums first, then the same sum over them
    std::vector<float> blocks(sah_blocks(n));
    for (uint32_t b = 0; b < blocks.size(); ++b) blocks[b] = sah_block_sum_host(terms.data() + (size_t)b * SAH_BLOCK, std::min(SAH_BLOCK, n - b * SAH_BLOCK));
    const float again = blocks.size() == 1 ? blocks[0] : sah_sum_host(blocks);
    CHECK(std::memcmp(&again, &sum, 4) == 0);
    // ... and sah_cost_host is that sum over a(root)
    const float cost = sah_cost_host(nodes, 0, entries), area = root_half_area(nodes[0]);
    const float want = area > 0.0f ? sum / area : 0.0f;
    CHECK(std::memcmp(&cost, &want, 4) == 0);
    return 0;
}

int check_hand_made() {
    // two leaves under one node: boxes 1 x 2 x 3 with 2 triangles and 2 x 2 x 2 with 3 triangles, side by side along x
    DevNode nd;
    std::memset(&nd, 0, sizeof(nd));
    const float lo0[3] = {0, 0, 0}, hi0[3] = {1, 2, 3}, lo1[3] = {1, 0, 0}, hi1[3] = {3, 2, 2};
    store_child_box(nd, 0, lo0, hi0); store_child_box(nd, 1, lo1, hi1);
    nd.child[0] = make_leaf(0, 2); nd.child[1] = make_leaf(2, 3);
    CHECK(half_area(lo0, hi0) == 11.0f && half_area(lo1, hi1) == 12.0f);              // 1*2 + 2*3 + 3*1; 2*2 + 2*2 + 2*2
    CHECK(root_half_area(nd) == 21.0f);                                                // the union is 3 x 2 x 3: 6 + 6 + 9
    CHECK(sah_cost_host({nd}, 0, {0u, 1u}) == (11.0f * 2.0f + 12.0f * 3.0f) / 21.0f);
    // a root that is a leaf: no node, no entry -> 0; so is a tree without extent
    CHECK(sah_cost_host({}, make_leaf(0, 3), {}) == 0.0f && sah_cost_host({nd}, 0, {}) == 0.0f);
    CHECK(sah_quotient(0.0f, 0.0f) == 0.0f);
    // the wrapped single leaf: the second child is the empty point box at +FLT_MAX, not used -> count of the leaf
    DevNode w = nd;
    const float far[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    store_child_box(w, 1, far, far); w.child[1] = w.child[0];
    CHECK(root_half_area(w) == 11.0f && sah_cost_host({w}, 0, {0u}) == 2.0f);
    // a chain of 40 nodes: node k holds a unit-cube leaf (1 triangle) and node k + 1, whose box is [0, 40 - k - 1] x 1 x 1
    const int len = 40;
    std::vector<DevNode> chain((size_t)len);
    std::vector<uint32_t> entries;
    long double sum = 0.0L;
    for (int k = len - 1; k >= 0; --k) {
        DevNode& c = chain[(size_t)k];
        std::memset(&c, 0, sizeof(c));
        const float l0[3] = {(float)(len - k - 1), 0, 0}, h0[3] = {(float)(len - k), 1, 1}, l1[3] = {0, 0, 0}, h1[3] = {(float)(len - k - 1), 1, 1};
        store_child_box(c, 0, l0, h0); c.child[0] = make_leaf((uint32_t)k, 1);
        if (k == len - 1) { store_child_box(c, 1, l0, h0); c.child[1] = make_leaf((uint32_t)len, 1); }
        else { store_child_box(c, 1, l1, h1); c.child[1] = k + 1; }
    }
    for (int k = len - 1; k >= 0; --k) for (uint32_t side = 0; side < 2; ++side) {     // lowest height first, like the plan
        entries.push_back(((uint32_t)k << 1) | side);
        sum += (long double)sah_term(chain[(size_t)k], (int)side);
    }
    const float cost = sah_cost_host(chain, 0, entries);                               // small integers: every addition is exact
    CHECK(cost == (float)sum / root_half_area(chain[0]) && root_half_area(chain[0]) == (float)(2 * len + 1));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s <seed> <n>\n", argv[0]); return 2; }
    rng.seed((uint32_t)std::atoi(argv[1]));
    const uint32_t n = (uint32_t)std::atoi(argv[2]);
    if (int rc = check_hand_made()) return rc;
    if (int rc = check_normals(400)) return rc;
    if (n) if (int rc = check_sums(n)) return rc;
    std::printf("ok %u\n", n);
    return 0;
}
