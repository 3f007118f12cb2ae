// Scene lowering: C-ABI description -> the host arrays of the flat HBM layout (layout.hpp).  Pure host C++ (scene_lower.hpp): what needs a
// device — the query, the optional GPU tree build, the upload — is scene.cpp.
#include "scene_lower.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "instance_move_plan.hpp"
#include "scene_edit_plan.hpp"

namespace pt {

namespace {

constexpr float PI_F = 3.14159265358979323846f;

struct V3 { float x, y, z; };
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
inline float length(V3 a) { return std::sqrt(dot(a, a)); }
inline V3 normalize(V3 a) { float r = 1.0f / length(a); return {a.x * r, a.y * r, a.z * r}; }
inline V3 vertex(const HostMesh& mesh, uint32_t v) { return V3{mesh.pos[3 * v], mesh.pos[3 * v + 1], mesh.pos[3 * v + 2]}; }
inline bool degenerate(V3 a, V3 b, V3 c) { const V3 cr = cross(b - a, c - a); return dot(cr, cr) == 0.0f; }

// the 9-float vertex block DevTri, DevTriLocal and DevLightTri share
template <typename Rec>
inline void set_vertices(Rec& r, V3 a, V3 b, V3 c) {
    r.p0[0] = a.x; r.p0[1] = a.y; r.p0[2] = a.z; r.p1x = b.x;
    r.p1yz[0] = b.y; r.p1yz[1] = b.z; r.p2xy[0] = c.x; r.p2xy[1] = c.y; r.p2z = c.z;
}

// column-major 4x4 * point (same operation order as glam::Mat4::transform_point3 so that light triangles
// and BVH triangles land on the very floats the reference computes in EmissiveTriangleMesh::sample_radiance)
inline V3 xform_point(const float* m, V3 p) {
    float r[4];
    for (int i = 0; i < 4; ++i) r[i] = m[i] * p.x;
    for (int i = 0; i < 4; ++i) r[i] = r[i] + m[4 + i] * p.y;
    for (int i = 0; i < 4; ++i) r[i] = r[i] + m[8 + i] * p.z;
    for (int i = 0; i < 4; ++i) r[i] = r[i] + m[12 + i];
    return {r[0], r[1], r[2]};
}
inline void mat4_mul(const float* a, const float* b, float* o) {   // o = a * b, column-major
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float s = a[r] * b[4 * c];
            s = s + a[4 + r] * b[4 * c + 1];
            s = s + a[8 + r] * b[4 * c + 2];
            s = s + a[12 + r] * b[4 * c + 3];
            o[4 * c + r] = s;
        }
}
// The linear part of a column-major 4x4 in double: a = that 3x3 (column-major), inv = its inverse (same layout).  Returns the determinant;
// with a zero determinant inv is not finite (lower_transform refuses such an instance).
inline double mat3_inverse(const float* m4, double a[9], double inv[9]) {
    const double l[9] = {m4[0], m4[1], m4[2], m4[4], m4[5], m4[6], m4[8], m4[9], m4[10]};
    for (int i = 0; i < 9; ++i) a[i] = l[i];
    const double det = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2]) + a[6] * (a[1] * a[5] - a[4] * a[2]);
    const double r[9] = {(a[4] * a[8] - a[7] * a[5]) / det, -(a[1] * a[8] - a[7] * a[2]) / det, (a[1] * a[5] - a[4] * a[2]) / det,
                         -(a[3] * a[8] - a[6] * a[5]) / det, (a[0] * a[8] - a[6] * a[2]) / det, -(a[0] * a[5] - a[3] * a[2]) / det,
                         (a[3] * a[7] - a[6] * a[4]) / det, -(a[0] * a[7] - a[6] * a[1]) / det, (a[0] * a[4] - a[3] * a[1]) / det};
    for (int i = 0; i < 9; ++i) inv[i] = r[i];
    return det;
}

// glam::Mat4::inverse (the cofactor form glam inherits from GLM), operation for operation: the device multiplies rays and hits with THESE
// floats where the reference inverts local_to_render in every intersect call (primitive/impls/triangle_mesh.rs:97,  math/src/transform.rs:159-162).
inline void mat4_inverse_glam(const float* s, float* o) {   // column-major 4x4
    const float m00 = s[0], m01 = s[1], m02 = s[2], m03 = s[3], m10 = s[4], m11 = s[5], m12 = s[6], m13 = s[7];
    const float m20 = s[8], m21 = s[9], m22 = s[10], m23 = s[11], m30 = s[12], m31 = s[13], m32 = s[14], m33 = s[15];
    const float coef00 = m22 * m33 - m32 * m23, coef02 = m12 * m33 - m32 * m13, coef03 = m12 * m23 - m22 * m13;
    const float coef04 = m21 * m33 - m31 * m23, coef06 = m11 * m33 - m31 * m13, coef07 = m11 * m23 - m21 * m13;
    const float coef08 = m21 * m32 - m31 * m22, coef10 = m11 * m32 - m31 * m12, coef11 = m11 * m22 - m21 * m12;
    const float coef12 = m20 * m33 - m30 * m23, coef14 = m10 * m33 - m30 * m13, coef15 = m10 * m23 - m20 * m13;
    const float coef16 = m20 * m32 - m30 * m22, coef18 = m10 * m32 - m30 * m12, coef19 = m10 * m22 - m20 * m12;
    const float coef20 = m20 * m31 - m30 * m21, coef22 = m10 * m31 - m30 * m11, coef23 = m10 * m21 - m20 * m11;
    const float fac0[4] = {coef00, coef00, coef02, coef03}, fac1[4] = {coef04, coef04, coef06, coef07}, fac2[4] = {coef08, coef08, coef10, coef11};
    const float fac3[4] = {coef12, coef12, coef14, coef15}, fac4[4] = {coef16, coef16, coef18, coef19}, fac5[4] = {coef20, coef20, coef22, coef23};
    const float vec0[4] = {m10, m00, m00, m00}, vec1[4] = {m11, m01, m01, m01}, vec2[4] = {m12, m02, m02, m02}, vec3[4] = {m13, m03, m03, m03};
    const float sa[4] = {1, -1, 1, -1}, sb[4] = {-1, 1, -1, 1};
    float inv[16];
    for (int i = 0; i < 4; ++i) {
        inv[i] = ((vec1[i] * fac0[i] - vec2[i] * fac1[i]) + vec3[i] * fac2[i]) * sa[i];
        inv[4 + i] = ((vec0[i] * fac0[i] - vec2[i] * fac3[i]) + vec3[i] * fac4[i]) * sb[i];
        inv[8 + i] = ((vec0[i] * fac1[i] - vec1[i] * fac3[i]) + vec3[i] * fac5[i]) * sa[i];
        inv[12 + i] = ((vec0[i] * fac2[i] - vec1[i] * fac4[i]) + vec2[i] * fac5[i]) * sb[i];
    }
    const float d0 = s[0] * inv[0], d1 = s[1] * inv[4], d2 = s[2] * inv[8], d3 = s[3] * inv[12];
    const float det = ((d0 + d1) + d2) + d3;
    const float rcp = 1.0f / det;
    for (int i = 0; i < 16; ++i) o[i] = inv[i] * rcp;
}

inline float srgb_eotf_inverse(float c) { return c <= 0.04045f ? c / 12.92f : std::pow((c + 0.055f) / 1.055f, 2.4f); }

// ---------------- stage A: description + camera -> geometry ----------------

// One delta or environment light enters the light list (creation order, interleaved with the emissive instances)
void lower_delta_light(const HostDeltaLight& hl, const float* w2r, LoweredGeometry* g) {
    DevLight dl{};
    dl.first_tri = 0; dl.n_tris = 0; dl.material = hl.material; dl.kind = hl.d.kind;   // LK_* == MI355PT_LIGHT_*
    dl.intensity = hl.d.intensity; dl.angle_inner = hl.d.angle_inner; dl.angle_outer = hl.d.angle_outer;
    float l2r[16];
    mat4_mul(w2r, hl.d.local_to_world, l2r);
    if (hl.d.kind == LK_ENV) {                                              // EnvironmentLight: phi = intensity * integrated spectrum
        dl.area_sum = hl.d.intensity;
        dl.first_tri = hl.env_index;                                        // DevScene::envs index
        g->env_light_index[hl.env_index] = (uint32_t)g->lights.size();
        std::memcpy(g->env_l2r[hl.env_index].data(), l2r, sizeof(float) * 16);
        g->lights.push_back(dl);
        return;
    }
    if (hl.d.kind == MI355PT_LIGHT_DIRECTIONAL) {
        V3 d = normalize(V3{l2r[8], l2r[9], l2r[10]});                        // local_to_render * (0,0,1), normalised
        dl.pos[0] = d.x; dl.pos[1] = d.y; dl.pos[2] = d.z;
    } else {
        dl.pos[0] = l2r[12]; dl.pos[1] = l2r[13]; dl.pos[2] = l2r[14];       // local_to_render * Point3::ZERO
        double a[9], inv[9];
        mat3_inverse(l2r, a, inv);
        // third row of the inverse: (inv * w).z (spot_light.rs:110)
        dl.axis[0] = (float)inv[2]; dl.axis[1] = (float)inv[5]; dl.axis[2] = (float)inv[8];
    }
    // phi's scalar factor ({point,spot,directional}_light.rs: phi()); the directional area is filled once the bounds are known
    if (hl.d.kind == MI355PT_LIGHT_POINT) dl.area_sum = 4.0f * PI_F * hl.d.intensity;
    else if (hl.d.kind == MI355PT_LIGHT_SPOT)   // ((I*s)*2*pi)*bracket in the reference; here s*(I*2*pi*bracket): same value up to rounding
        dl.area_sum = hl.d.intensity * 2.0f * PI_F * ((1.0f - std::cos(hl.d.angle_inner)) + (std::cos(hl.d.angle_inner) - std::cos(hl.d.angle_outer)) / 2.0f);
    g->lights.push_back(dl);
}

// primitive bounds = the mesh's local AABB carried through local_to_render (primitive/impls/triangle_mesh.rs:62-70), joined to the scene's
void mesh_aabb(const HostMesh& mesh, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t v = 0; v < mesh.n_vert; ++v) for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], mesh.pos[3 * v + a]); hi[a] = std::fmax(hi[a], mesh.pos[3 * v + a]); }
}
void grow_scene_bounds(const float lo[3], const float hi[3], const float* l2r, float sb_lo[3], float sb_hi[3]) {
    for (int k = 0; k < 8; ++k) {
        V3 q = xform_point(l2r, V3{(k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]});
        sb_lo[0] = std::fmin(sb_lo[0], q.x); sb_lo[1] = std::fmin(sb_lo[1], q.y); sb_lo[2] = std::fmin(sb_lo[2], q.z);
        sb_hi[0] = std::fmax(sb_hi[0], q.x); sb_hi[1] = std::fmax(sb_hi[1], q.y); sb_hi[2] = std::fmax(sb_hi[2], q.z);
    }
}

// The instance's two matrices and whether both are a pure translation
bool lower_transform(const float* l2r, int lowering, bool dynamic, DevInstance* di) {
    double a[9], inv3[9];
    if (mat3_inverse(l2r, a, inv3) == 0.0) return false;
    float inv[16];
    mat4_inverse_glam(l2r, inv);
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) { di->m[3 * c + r] = l2r[4 * c + r]; di->inv[3 * c + r] = inv[4 * c + r]; }
    for (int k = 0; k < 12; ++k) if (!std::isfinite(di->inv[k])) return false;
    // a pure translation: both 3x3 parts equal the identity NUMERICALLY (glam's inverse of a translation holds -0.0 in some off-diagonal
    // entries; a * 1 + b * (-0) + c * 0 is still a, up to the sign of a zero, which no later operation can see)
    di->identity = 1u;
    for (int k = 0; k < 9; ++k) { const float e = (k % 4 == 0) ? 1.0f : 0.0f; if (!(di->m[k] == e) || !(di->inv[k] == e)) di->identity = 0u; }
    if (lowering >= 2) di->identity = 0u;                                 // (mi355pt_scene_debug_set_lowering: every instance through the general matrix path)
    if (dynamic) di->identity = 0u;                                       // (mi355pt_scene_set_instance_dynamic: this one through it, whatever it is moved to)
    di->pad[0] = di->pad[1] = di->pad[2] = 0;
    return true;
}

// EmissiveTriangleMesh::new: areas in WORLD space, their sum and the normalised running sums (emissive_triangle_mesh.rs:28-68)
struct AreaTables { std::vector<float> area, cdf; float sum = 0.0f; };
AreaTables area_light_tables(const HostMesh& mesh, const float* l2w) {
    AreaTables t;
    for (uint32_t k = 0; k < mesh.n_tri; ++k) {
        V3 p[3];
        for (int j = 0; j < 3; ++j) p[j] = xform_point(l2w, vertex(mesh, mesh.idx[3 * k + j]));
        V3 e0 = p[0] - p[1], e1 = p[0] - p[2];
        t.area.push_back(length(cross(e0, e1)) * 0.5f);
    }
    for (float a : t.area) { t.sum += a; t.cdf.push_back(t.sum); }
    for (float& a : t.cdf) a /= t.sum;
    return t;
}

inline EditMaterialKey material_key(const DevMaterial& m) { return EditMaterialKey{m.type, m.color.kind, m.cc_tint.kind, m.eta.kind}; }

// The records of one instance's triangles, in mesh order; `areas`: the instance is an area light, `light_index` its place in the light list
void lower_triangles(const SceneImpl& scene, uint32_t ii, const float* l2r, const DevInstance& di, const AreaTables* areas, uint32_t light_index,
                     LoweredGeometry* g, std::vector<uint8_t>* deg_render, std::vector<uint8_t>* deg_local) {
    const HostInstance& inst = scene.instances[ii];
    const HostMesh& mesh = scene.meshes[inst.geom];
    // sort class of the deferral queue (pt_kernel.hpp), stated in scene_edit_plan.hpp: an edit of the material recomputes it (reclass_tris_kernel)
    const uint32_t mclass = edit_material_class(material_key(scene.materials[inst.mat]));
    for (uint32_t t = 0; t < mesh.n_tri; ++t) {
        const uint32_t vi[3] = {mesh.idx[3 * t], mesh.idx[3 * t + 1], mesh.idx[3 * t + 2]};
        V3 p[3], pl[3];
        for (int k = 0; k < 3; ++k) { pl[k] = vertex(mesh, vi[k]); p[k] = xform_point(l2r, pl[k]); }
        DevTri dt{};
        set_vertices(dt, p[0], p[1], p[2]);
        dt.mclass = mclass; dt.instance = ii; dt.flags = di.identity;
        g->tris.push_back(dt);
        DevTriLocal tl{};
        set_vertices(tl, pl[0], pl[1], pl[2]);
        tl.instance = ii; tl.flags = di.identity; tl.mclass = mclass;
        g->tris_local.push_back(tl);
        BuildTri bt;
        for (int a = 0; a < 3; ++a) {
            float v0 = (&p[0].x)[a], v1 = (&p[1].x)[a], v2 = (&p[2].x)[a];
            bt.lo[a] = std::fmin(v0, std::fmin(v1, v2)); bt.hi[a] = std::fmax(v0, std::fmax(v1, v2));
            bt.c[a] = 0.5f * (bt.lo[a] + bt.hi[a]);
        }
        g->build_tris.push_back(bt);
        // math::intersect_triangle rejects a triangle whose cross product is exactly zero (ray.rs:49-56) before anything else: such a
        // triangle can never be hit, so it stays out of the tree and the traversals' triangle test does not repeat the check for every
        // candidate (pt_device.hpp intersect_triangle<false>: +1.5 % on the Cornell scenes, +5 % on the 20 k-triangle hero of scene 17).
        // Decided on the vertices the traversal will test, with the device's arithmetic.
        deg_render->push_back(degenerate(p[0], p[1], p[2]) ? 1 : 0);
        deg_local->push_back(degenerate(pl[0], pl[1], pl[2]) ? 1 : 0);

        DevTriShade sh{};
        {   // the hit's geometric normal is a function of the triangle alone: ray.rs:167-174 in LOCAL space, then Transform * Normal
            // (samples.rs:135, transform.rs:45-51: transpose(inverse) * n, renormalised) - computed here once with the arithmetic of the
            // device code it replaces (xf_normal, pt_device.hpp; a translation leaves normalize(n)).  instance_move_plan.hpp holds the
            // expression: an instance move recomputes it on the device (shade_refresh_kernel)
            const IV3 n = shade_normal(IV3{pl[0].x, pl[0].y, pl[0].z}, IV3{pl[1].x, pl[1].y, pl[1].z}, IV3{pl[2].x, pl[2].y, pl[2].z}, di.inv, di.identity != 0u);
            sh.ng[0] = n.x; sh.ng[1] = n.y; sh.ng[2] = n.z; sh.pad_ng = 0;
        }
        const float* n0 = &mesh.nrm[3 * vi[0]]; const float* n1 = &mesh.nrm[3 * vi[1]]; const float* n2 = &mesh.nrm[3 * vi[2]];
        sh.n0[0] = n0[0]; sh.n0[1] = n0[1]; sh.n0[2] = n0[2]; sh.n1x = n1[0];
        sh.n1yz[0] = n1[1]; sh.n1yz[1] = n1[2]; sh.n2xy[0] = n2[0]; sh.n2xy[1] = n2[1]; sh.n2z = n2[2];
        sh.flags = di.identity ? 4u : 0u;                                      // bit 2: the instance's linear part is the identity (load_surface)
        if (!mesh.uv.empty()) {
            sh.flags |= 1u;
            sh.tangent[0] = mesh.tangent[3 * t]; sh.tangent[1] = mesh.tangent[3 * t + 1]; sh.tangent[2] = mesh.tangent[3 * t + 2];
            sh.uv0[0] = mesh.uv[2 * vi[0]]; sh.uv0[1] = mesh.uv[2 * vi[0] + 1];
            sh.uv1[0] = mesh.uv[2 * vi[1]]; sh.uv1[1] = mesh.uv[2 * vi[1] + 1];
            sh.uv2[0] = mesh.uv[2 * vi[2]]; sh.uv2[1] = mesh.uv[2 * vi[2] + 1];
        }
        sh.material = inst.mat; sh.instance = ii; sh.local_tri = t; sh.light = light_index;
        sh.light_pdf_area = 0.0f;
        if (areas) {
            sh.flags |= 2u;
            sh.light_pdf_area = light_pdf_area_of(areas->area, areas->cdf, t);            // :334-353
            DevLightTri lt{};
            set_vertices(lt, p[0], p[1], p[2]);                                  // sample_radiance transforms the ORIGINAL vertex order with local_to_render (:200-206)
            lt.cdf = areas->cdf[t];
            { V3 n = normalize(normalize(cross(p[1] - p[0], p[2] - p[0]))); lt.n[0] = n.x; lt.n[1] = n.y; lt.n[2] = n.z; }
            g->light_tris.push_back(lt);
            for (int k = 0; k < 3; ++k) {
                g->light_uvs.push_back(mesh.uv.empty() ? 0.0f : mesh.uv[2 * vi[k]]); g->light_uvs.push_back(mesh.uv.empty() ? 0.0f : mesh.uv[2 * vi[k] + 1]);
            }
        }
        g->shade.push_back(sh);
    }
}

// DirectionalLight::preprocess (directional_light.rs:46-54): area = pi r^2 of the scene's bounding sphere (bounds.rs:59-77)
void set_directional_areas(const float sb_lo[3], const float sb_hi[3], std::vector<DevLight>* lights) {
    V3 c{(sb_lo[0] + sb_hi[0]) * 0.5f, (sb_lo[1] + sb_hi[1]) * 0.5f, (sb_lo[2] + sb_hi[2]) * 0.5f};
    float radius = length(V3{c.x - sb_hi[0], c.y - sb_hi[1], c.z - sb_hi[2]});
    for (DevLight& dl : *lights) {
        if (dl.kind == LK_DIRECTIONAL) dl.area_sum = dl.intensity * (PI_F * radius * radius);
    }
}

// The builder's input: the bounds of the triangles that can be hit, and which triangle each is
void filter_degenerate(const std::vector<uint8_t>& deg, LoweredGeometry* g) {
    std::vector<BuildTri> keep_b;
    for (size_t i = 0; i < g->build_tris.size(); ++i) if (!deg[i]) { g->kept.push_back((uint32_t)i); keep_b.push_back(g->build_tris[i]); }
    g->n_degenerate = g->build_tris.size() - g->kept.size();
    g->build_tris.swap(keep_b);
}

// ---------------- stage B: geometry + BVH2 -> everything in leaf order, the tables, the scalars ----------------

void reorder_to_leaves(const LoweredGeometry& g, const std::vector<uint32_t>& order, LoweredScene* ls) {
    ls->tris_render.resize(order.size()); ls->shade.resize(order.size()); ls->tris_local.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) { const uint32_t t = g.kept[order[i]]; ls->tris_render[i] = g.tris[t]; ls->shade[i] = g.shade[t]; ls->tris_local[i] = g.tris_local[t]; }
}

// LUT pool, CMF, the rgb2spec table repacked to float4 cells + its z nodes
void pack_spectral_tables(const SceneImpl& scene, const float* cmf4, LoweredScene* ls) {
    for (auto& l : scene.luts) ls->luts.insert(ls->luts.end(), l.begin(), l.end());
    ls->cmf.assign(cmf4, cmf4 + 470 * 4);
    const std::vector<float>& table = scene.table;
    if (table.empty()) return;
    const size_t cells = (size_t)3 * 64 * 64 * 64;
    std::vector<float>& tab4 = ls->rgb2spec;
    tab4.resize(cells * 4);
    for (size_t c = 0; c < cells; ++c) { tab4[4 * c] = table[64 + 3 * c]; tab4[4 * c + 1] = table[64 + 3 * c + 1]; tab4[4 * c + 2] = table[64 + 3 * c + 2]; tab4[4 * c + 3] = 0.0f; }
    ls->z_nodes.assign(table.begin(), table.begin() + 64);
}

// textures as one RGBA8 pool + their descriptors
void pack_textures(const SceneImpl& scene, LoweredScene* ls) {
    for (auto& t : scene.textures) {
        ls->textures.push_back(DevTexture{(uint32_t)ls->texels.size(), t.w, t.h, 0});
        size_t n = (size_t)t.w * t.h;
        for (size_t i = 0; i < n; ++i) ls->texels.push_back((uint32_t)t.rgb[3 * i] | ((uint32_t)t.rgb[3 * i + 1] << 8) | ((uint32_t)t.rgb[3 * i + 2] << 16));
    }
}

// EnvironmentLight::new (environment_light.rs:28-75) + build_2d_cdf (:153-199): one light's tables, its DevEnv record and the integrated
// spectrum of its hidden emissive material `hm` (an entry of the LOWERED materials: the description stays as it is)
int lower_environment(const SceneImpl& scene, const SceneImpl::HostEnv& env, const float* l2r, uint32_t light_index, LoweredScene::EnvTables* tab,
                      DevEnv* denv, DevMaterial* hm, std::string* err) {
    if (scene.table.empty()) { *err = "environment light needs the rgb2spec table"; return MI355PT_E_INVALID; }
    const uint32_t w = env.w, h = env.h;
    float tot[3] = {0, 0, 0};
    tab->texels.resize((size_t)w * h * 4);
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) {
        const float* p = &env.rgb[((size_t)y * w + x) * 3];
        for (int c = 0; c < 3; ++c) { tot[c] += p[c]; tab->texels[((size_t)y * w + x) * 4 + c] = p[c]; }
        tab->texels[((size_t)y * w + x) * 4 + 3] = 0.0f;
    }
    float n = (float)(w * h);
    for (int c = 0; c < 3; ++c) tot[c] /= n;
    float scale = 2.0f * std::fmax(tot[0], std::fmax(tot[1], tot[2]));       // integrated RgbIlluminantSpectrum (rgb_illuminant_spectrum.rs:26-41)
    if (scale == 0.0f) { hm->color.kind = SPK_CONSTANT; hm->color.c[0] = 0.0f; }
    else {
        float enc[3] = {tot[0] / scale, tot[1] / scale, tot[2] / scale};
        hm->color.kind = SPK_ILLUM; hm->color.id = env.illuminant_lut;
        if (!scene.table_lookup_srgb(enc, hm->color.c)) { *err = "rgb2spec lookup failed"; return MI355PT_E_INVALID; }
        std::memcpy(&hm->color.pad[0], &scale, sizeof(float));
    }
    std::vector<float> row_w(h, 0.0f);
    tab->conditional.assign((size_t)w * h, 0.0f); tab->marginal.assign(h, 0.0f);
    for (uint32_t y = 0; y < h; ++y) {
        float row_sum = 0.0f;
        for (uint32_t x = 0; x < w; ++x) {
            float v = ((float)y + 0.5f) / (float)h;
            float theta = v * PI_F;
            const float* p = &env.rgb[((size_t)y * w + x) * 3];
            float lum = 0.299f * p[0] + 0.587f * p[1] + 0.114f * p[2];
            row_sum += lum * std::fmax(std::sin(theta), 1e-8f);
            tab->conditional[(size_t)y * w + x] = row_sum;
        }
        row_w[y] = row_sum;
        if (row_sum > 0.0f) for (uint32_t x = 0; x < w; ++x) tab->conditional[(size_t)y * w + x] /= row_sum;
    }
    float total = 0.0f;
    for (float r : row_w) total += r;
    float cum = 0.0f;
    for (uint32_t y = 0; y < h; ++y) { cum += row_w[y]; tab->marginal[y] = total > 0.0f ? cum / total : (float)(y + 1) / (float)h; }
    denv->w = w; denv->h = h; denv->total_weight = total; denv->intensity = env.intensity; denv->illuminant_lut = env.illuminant_lut;
    denv->light_index = light_index;
    double a[9], inv[9];
    mat3_inverse(l2r, a, inv);
    for (int i = 0; i < 9; ++i) { denv->l2r[i] = (float)a[i]; denv->r2l[i] = (float)inv[i]; }
    return MI355PT_OK;
}

// The device copy of the materials: texture descriptors ride in the records that name the texture (layout.hpp), and every clearcoat
// material gets the coat's directional-albedo table (mi355pt_params.albedo_lut) and names its offset
// `reuse` (an edit of a built scene, lower_edit_records): a clearcoat material that is not marked in reuse->changed and was a clearcoat
// material in reuse->materials takes its row from reuse->cc_albedo — the row is a function of the record — instead of integrating it again
struct CoatRows { const std::vector<DevMaterial>& materials; const std::vector<float>& cc_albedo; const uint8_t* changed; };
void finish_materials(LoweredScene* ls, const CoatRows* reuse = nullptr) {
    for (size_t mi = 0; mi < ls->materials.size(); ++mi) {
        DevMaterial& m = ls->materials[mi];
        m.normal_desc = m.normal_tex != 0xffffffffu ? ls->textures[m.normal_tex] : DevTexture{0, 0, 0, 0};
        for (DevSpectrum* sp : {&m.color, &m.eta, &m.cc_tint})
            if (sp->kind == SPK_TEXTURE) { const DevTexture& t = ls->textures[sp->id]; sp->pad[0] = t.offset; sp->pad[1] = t.w; sp->pad[2] = t.h; }
        m.cc_albedo_lut = 0;
        if (m.type != MT_CLEARCOAT) continue;
        float r = (m.cc_ior - 1.0f) / (m.cc_ior + 1.0f);
        m.cc_albedo_lut = (uint32_t)ls->cc_albedo.size();
        ls->cc_albedo.resize(ls->cc_albedo.size() + 64);
        if (reuse && !reuse->changed[mi] && mi < reuse->materials.size() && reuse->materials[mi].type == MT_CLEARCOAT &&
            (size_t)reuse->materials[mi].cc_albedo_lut + 64 <= reuse->cc_albedo.size())
            std::memcpy(ls->cc_albedo.data() + m.cc_albedo_lut, reuse->cc_albedo.data() + reuse->materials[mi].cc_albedo_lut, 64 * sizeof(float));
        else
            coat_albedo_table(m.cc_roughness * m.cc_roughness, r * r, ls->cc_albedo.data() + m.cc_albedo_lut);
    }
    if (ls->cc_albedo.empty()) ls->cc_albedo.assign(64, 0.0f);
}

uint32_t scene_features(const SceneImpl& scene, size_t n_lights) {
    uint32_t features = n_lights == 1 ? 0u : FEAT_MLIGHT;
    if (!scene.delta_lights.empty()) features |= FEAT_DELTA;
    if (!scene.envs.empty()) features |= FEAT_ENV;
    for (const HostInstance& inst : scene.instances) {
        const DevMaterial& m = scene.materials[inst.mat];
        if (m.type == MT_GLASS || m.type == MT_PLASTIC) features |= FEAT_DIEL | ((m.roughness >= 1e-3f || m.roughness_tex != 0xffffffffu) ? FEAT_ROUGH : 0u);
        if (m.type == MT_CLEARCOAT) features |= FEAT_CC;
        if (m.type == MT_METAL) features |= FEAT_METAL;
        if (m.type == MT_EMISSIVE && (m.color.kind == SPK_TEXTURE || m.metallic_tex != 0xffffffffu)) features |= FEAT_EMTEX;   // textured radiance or intensity
        if (m.normal_tex != 0xffffffffu || m.color.kind == SPK_TEXTURE || m.cc_tint.kind == SPK_TEXTURE || m.metallic_tex != 0xffffffffu ||
            m.roughness_tex != 0xffffffffu || m.cc_thickness_tex != 0xffffffffu) features |= FEAT_TEX;
    }
    return features;
}

// ---------------- the 4-wide tree ----------------

inline bool slot_used(const DevNode4& n, int c) { return n.lox[c] <= n.hix[c] && n.lox[c] < FLT_MAX; }   // unused slots: point boxes at FLT_MAX

#if PT_NODE_FMA
// pad the boxes the fma slab test sees (layout.hpp PT_NODE_FMA); unused slots stay as they are
void pad_nodes4(std::vector<DevNode4>* nodes4) {
    const float pad = nodes4_pad_radius(*nodes4) * NODE4_PAD_REL;
    for (DevNode4& n : *nodes4) for (int c = 0; c < 4; ++c) if (slot_used(n, c)) {
        n.lox[c] -= pad; n.loy[c] -= pad; n.loz[c] -= pad; n.hix[c] += pad; n.hiy[c] += pad; n.hiz[c] += pad;
    }
}
#endif

#if PT_NODE_Q16
// the boxes on the 16-bit scene grid (layout.hpp PT_NODE_Q16): lo planes down, hi planes up, checked against the float boxes
bool quantise_nodes4(const std::vector<DevNode4>& nodes4, float grid_org[3], float grid_cell[3], std::vector<DevNode4Q>* q4, std::string* err) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (const DevNode4& n : nodes4) for (int c = 0; c < 4; ++c) if (slot_used(n, c)) {
        const float l[3] = {n.lox[c], n.loy[c], n.loz[c]}, h[3] = {n.hix[c], n.hiy[c], n.hiz[c]};
        for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], l[a]); hi[a] = std::fmax(hi[a], h[a]); }
    }
    float rmax = 0.0f;
    for (int a = 0; a < 3; ++a) rmax = std::fmax(rmax, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
    // the fma slab test is off by up to 2 u max(|o|, |plane|) in space (layout.hpp PT_NODE_FMA): every plane moves out by `pad` more
    const float pad = rmax * NODE4_PAD_REL;
    for (int a = 0; a < 3; ++a) {
        const float ext = std::fmax(hi[a] - lo[a], 1e-20f) + 4.0f * pad;
        grid_org[a] = lo[a] - 2.0f * pad;
        grid_cell[a] = ext / 65533.0f;
    }
    q4->resize(nodes4.size());
    for (size_t i = 0; i < nodes4.size(); ++i) {
        const DevNode4& n = nodes4[i]; DevNode4Q& q = (*q4)[i];
        for (int c = 0; c < 4; ++c) {
            q.child[c] = n.child[c];
            const float l[3] = {n.lox[c], n.loy[c], n.loz[c]}, h[3] = {n.hix[c], n.hiy[c], n.hiz[c]};
            for (int a = 0; a < 3; ++a) {
                if (!slot_used(n, c)) { q.q[a][0][c] = 65535; q.q[a][1][c] = 0; continue; }
                const float org = grid_org[a], cell = grid_cell[a];
                long ql = (long)std::floor((l[a] - pad - org) / cell), qh = (long)std::ceil((h[a] + pad - org) / cell);
                ql = std::min<long>(std::max<long>(ql, 0), 65535); qh = std::min<long>(std::max<long>(qh, 0), 65535);
                // in the arithmetic the kernel sees (origin + q * cell in f32): the quantised planes enclose the padded box
                while (ql > 0 && org + (float)ql * cell > l[a] - pad) --ql;
                while (qh < 65535 && org + (float)qh * cell < h[a] + pad) ++qh;
                if (org + (float)ql * cell > l[a] || org + (float)qh * cell < h[a]) { *err = "internal error: quantised BVH box does not enclose its box"; return false; }
                q.q[a][0][c] = (uint16_t)ql; q.q[a][1][c] = (uint16_t)qh;
            }
        }
    }
    return true;
}
#endif

inline uint64_t fnv1a64(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

}  // namespace

// the largest coordinate magnitude over the used slots: what pad_nodes4 scales its pad by
float nodes4_pad_radius(const std::vector<DevNode4>& nodes4) {
    float r = 0.0f;
    for (const DevNode4& n : nodes4) for (int c = 0; c < 4; ++c) if (n.lox[c] <= n.hix[c] && n.lox[c] < FLT_MAX)
        for (float v : {n.lox[c], n.loy[c], n.loz[c], n.hix[c], n.hiy[c], n.hiz[c]}) r = std::max(r, std::fabs(v));
    return r;
}

// ---------------- spectra and tables of the description (SceneImpl's const helpers) ----------------

bool SceneImpl::table_lookup_srgb(const float enc[3], float c[3], bool linear) const {
    const int TBL = 64;
    if (table.size() != (size_t)(TBL + 3 * TBL * TBL * TBL * 3)) return false;
    float rgb[3];
    for (int i = 0; i < 3; ++i) rgb[i] = std::fmax(linear ? enc[i] : srgb_eotf_inverse(enc[i]), 0.0f);   // color.invert_eotf() (:96-97)
    if (rgb[0] == rgb[1] && rgb[1] == rgb[2]) { c[0] = 0; c[1] = 0; c[2] = std::log(rgb[0] / (1.0f - rgb[0])); return true; }
    int mc = 0; float mx = rgb[0];
    if (rgb[1] > mx) { mx = rgb[1]; mc = 1; }
    if (rgb[2] > mx) { mc = 2; }
    float z = rgb[mc];
    float x = rgb[(mc + 1) % 3] * 63.0f / z, y = rgb[(mc + 2) % 3] * 63.0f / z;
    int xi = std::min((int)x, TBL - 2), yi = std::min((int)y, TBL - 2), zi = TBL - 2;
    for (int i = 0; i <= TBL - 2; ++i) if (table[i + 1] > z) { zi = i; break; }
    float dx = x - (float)xi, dy = y - (float)yi, dz = (z - table[zi]) / (table[zi + 1] - table[zi]);
    auto co = [&](int ddx, int ddy, int ddz, int k) {
        return table[TBL + ((((size_t)mc * TBL + zi + ddz) * TBL + yi + ddy) * TBL + xi + ddx) * 3 + k];
    };
    auto lerp = [](float a, float b, float t) { return a + (b - a) * t; };
    for (int k = 0; k < 3; ++k)
        c[k] = lerp(lerp(lerp(co(0, 0, 0, k), co(1, 0, 0, k), dx), lerp(co(0, 1, 0, k), co(1, 1, 0, k), dx), dy),
                    lerp(lerp(co(0, 0, 1, k), co(1, 0, 1, k), dx), lerp(co(0, 1, 1, k), co(1, 1, 1, k), dx), dy), dz);
    return true;
}

// Expectation of GeneralizedSchlickBsdf::directional_albedo's estimator (generalized_schlick.rs:893-918) for ScatterMode::R, a scalar r0,
// r90 = 1, exponent 5, tint 1 and alpha_x = alpha_y = alpha: mean over (u, v) in [0,1)^2 of f |cos i| / pdf with wi drawn by the GGX
// visible-normal sampler (:165-199) — the quantity the reference estimates with 64 random points per call.  Double precision, 256 x 256
// midpoints: deterministic, error ~1e-5 (the 64-point estimate it replaces has a standard deviation of 1e-2 .. 1e-1).
void coat_albedo_table(float alpha_f, float r0_f, float out[64]) {
    const double a = alpha_f, r0 = r0_f, PI = 3.14159265358979323846;
    auto lambda = [&](double x, double y, double z) { double c2 = z * z; if (c2 == 0.0) return 0.0; return (std::sqrt(1.0 + a * a * (x * x + y * y) / c2) - 1.0) / 2.0; };
    auto D = [&](double x, double y, double z) { double c2 = z * z; if (c2 == 0.0) return 0.0; double e = (x * x + y * y) / c2 / (a * a); return 1.0 / (PI * a * a * c2 * c2 * (1.0 + e) * (1.0 + e)); };
    for (int k = 0; k < 64; ++k) {
        const double cz = (k + 0.5) / 64.0, sx = std::sqrt(std::max(1.0 - cz * cz, 0.0));     // wo = (sin, 0, cos): the estimate is isotropic in wo
        const double wo[3] = {sx, 0.0, cz};
        double sum = 0.0;
        const int N = 256;
        for (int iu = 0; iu < N; ++iu) for (int iv = 0; iv < N; ++iv) {
            const double u = (iu + 0.5) / N, v = (iv + 0.5) / N;
            double term = 0.0;
            if (a < 1e-3) {                                                     // effectively smooth: wi = mirror, f = F, pdf = 1 (:232-251)
                double o = 1.0 - std::min(std::max(cz, 0.0), 1.0);
                term = (r0 + (1.0 - r0) * o * o * o * o * o) * cz;
            } else {
                double wh[3] = {a * wo[0], a * wo[1], wo[2]};
                double l = std::sqrt(wh[0] * wh[0] + wh[1] * wh[1] + wh[2] * wh[2]); wh[0] /= l; wh[1] /= l; wh[2] /= l;
                double t1[3] = {1, 0, 0};
                if (wh[2] < 0.99999) { double tl = std::sqrt(wh[0] * wh[0] + wh[1] * wh[1]); t1[0] = -wh[1] / tl; t1[1] = wh[0] / tl; t1[2] = 0.0; }
                const double t2[3] = {wh[1] * t1[2] - wh[2] * t1[1], wh[2] * t1[0] - wh[0] * t1[2], wh[0] * t1[1] - wh[1] * t1[0]};
                const double r = std::sqrt(u), th = 2.0 * PI * v;
                const double px = r * std::cos(th), pyy = r * std::sin(th);
                const double h = std::sqrt(std::max(1.0 - px * px, 0.0)), lf = (1.0 + wh[2]) / 2.0;
                const double py = h * (1.0 - lf) + pyy * lf, pz = std::sqrt(std::max(1.0 - px * px - py * py, 0.0));
                double nh[3] = {t1[0] * px + t2[0] * py + wh[0] * pz, t1[1] * px + t2[1] * py + wh[1] * pz, t1[2] * px + t2[2] * py + wh[2] * pz};
                double wm[3] = {a * nh[0], a * nh[1], std::max(1e-6, nh[2])};
                l = std::sqrt(wm[0] * wm[0] + wm[1] * wm[1] + wm[2] * wm[2]); wm[0] /= l; wm[1] /= l; wm[2] /= l;
                const double wodm = wo[0] * wm[0] + wo[1] * wm[1] + wo[2] * wm[2];
                const double wi[3] = {2.0 * wodm * wm[0] - wo[0], 2.0 * wodm * wm[1] - wo[1], 2.0 * wodm * wm[2] - wo[2]};
                const double cd = std::fabs(wodm), ci = std::fabs(wi[2]);
                if (wo[2] * wi[2] > 0.0 && cd >= 1e-6 && ci > 0.0) {
                    const double d = D(wm[0], wm[1], wm[2]);
                    const double pdf = (1.0 / (1.0 + lambda(wo[0], wo[1], wo[2]))) / cz * d * cd / (4.0 * cd);
                    const double g = 1.0 / (1.0 + lambda(wo[0], wo[1], wo[2]) + lambda(wi[0], wi[1], wi[2]));
                    const double o = 1.0 - std::min(std::max(cd, 0.0), 1.0);
                    const double f = (r0 + (1.0 - r0) * o * o * o * o * o) * d * g / (4.0 * cz);
                    if (pdf > 0.0) term = f * ci / pdf;
                }
            }
            sum += term;
        }
        out[k] = (float)(sum / ((double)N * N));
    }
}

int SceneImpl::lower_spectrum(const mi355pt_spectrum& in, DevSpectrum* out, int allow_texture, std::string* err) const {
    std::memset(out, 0, sizeof(*out));
    switch (in.kind) {
        case MI355PT_SPEC_CONSTANT: out->kind = SPK_CONSTANT; out->c[0] = in.c[0]; return MI355PT_OK;
        case MI355PT_SPEC_SIGMOID: out->kind = SPK_SIGMOID; std::memcpy(out->c, in.c, 12); return MI355PT_OK;
        case MI355PT_SPEC_RGB_ALBEDO_SRGB:
            if (!table_lookup_srgb(in.c, out->c)) { *err = "RGB spectrum needs mi355pt_scene_set_rgb2spec first"; return MI355PT_E_INVALID; }
            out->kind = SPK_SIGMOID; return MI355PT_OK;
        case MI355PT_SPEC_RGB_ALBEDO_SRGB_LINEAR:
            if (!table_lookup_srgb(in.c, out->c, true)) { *err = "RGB spectrum needs mi355pt_scene_set_rgb2spec first"; return MI355PT_E_INVALID; }
            out->kind = SPK_SIGMOID; return MI355PT_OK;
        case MI355PT_SPEC_LUT470:
            if (in.id >= luts.size()) { *err = "bad LUT id"; return MI355PT_E_INVALID; }
            out->kind = SPK_LUT; out->id = in.id; return MI355PT_OK;
        case MI355PT_SPEC_TEXTURE_ALBEDO_SRGB:
            if (!allow_texture) { *err = "texture spectrum not supported for this parameter"; return MI355PT_E_INVALID; }
            if (in.id >= textures.size() || table.empty()) { *err = "bad texture id or missing rgb2spec table"; return MI355PT_E_INVALID; }
            out->kind = SPK_TEXTURE; out->id = in.id; return MI355PT_OK;
        case MI355PT_SPEC_TEXTURE_ILLUMINANT_SRGB:
        case MI355PT_SPEC_TEXTURE_UNBOUNDED_SRGB: {
            // SpectrumType::{Illuminant, Unbounded} (rgb_texture.rs:56-64): the emitters' types
            if (allow_texture < 2) { *err = "Illuminant / Unbounded texture spectra are accepted for emitter radiance only"; return MI355PT_E_INVALID; }
            if (in.id >= textures.size() || table.empty()) { *err = "bad texture id or missing rgb2spec table"; return MI355PT_E_INVALID; }
            const uint32_t sub = in.kind == MI355PT_SPEC_TEXTURE_ILLUMINANT_SRGB ? 1u : 2u, lut = (uint32_t)in.c[0];
            if (sub == 1u && (!(in.c[0] >= 0.0f) || lut >= luts.size())) { *err = "Illuminant texture: c[0] must hold the LUT470 id of the illuminant"; return MI355PT_E_INVALID; }
            out->kind = SPK_TEXTURE; out->id = in.id;
            std::memcpy(&out->c[0], &sub, 4); std::memcpy(&out->c[1], &lut, 4);
            return MI355PT_OK;
        }
        default: *err = "unknown spectrum kind"; return MI355PT_E_INVALID;
    }
}

// ---------------- the stages ----------------

int lower_geometry(const SceneImpl& scene, const mi355pt_camera* cam, LoweredGeometry* g, std::string* err) {
    if (scene.instances.empty()) { *err = "scene has no instances"; return MI355PT_E_INVALID; }
    // world -> render = translate(-camera position)  (camera.rs:84-86, scene.rs:65-66)
    const float w2r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -cam->position[0], -cam->position[1], -cam->position[2], 1};
    *g = LoweredGeometry{};
    g->instances.resize(scene.instances.size());
    g->env_light_index.assign(scene.envs.size(), 0u);
    g->env_l2r.resize(scene.envs.size());
    std::vector<uint8_t> deg_render, deg_local;      // cross product exactly zero (render-space / local vertices)
    bool all_shared = true, have_shared = false;
    float sb_lo[3] = {INFINITY, INFINITY, INFINITY}, sb_hi[3] = {-INFINITY, -INFINITY, -INFINITY};   // scene bounds (render space)
    const std::vector<HostDeltaLight>& delta = scene.delta_lights;
    size_t next_delta = 0;
    for (size_t ii = 0; ii < scene.instances.size(); ++ii) {
        while (next_delta < delta.size() && delta[next_delta].after_instances <= ii) lower_delta_light(delta[next_delta++], w2r, g);
        const HostInstance& inst = scene.instances[ii];
        const HostMesh& mesh = scene.meshes[inst.geom];
        float l2r[16];
        mat4_mul(w2r, inst.l2w, l2r);                                          // triangle_mesh.rs:38-40
        { float lo[3], hi[3]; mesh_aabb(mesh, lo, hi); grow_scene_bounds(lo, hi, l2r, sb_lo, sb_hi); }
        DevInstance& di = g->instances[ii];
        if (!lower_transform(l2r, scene.lowering, inst.dynamic != 0u, &di)) { *err = "singular instance transform"; return MI355PT_E_INVALID; }
        // do all instances share ONE pure translation?  (DevScene::tris_are_local)
        if (!di.identity) all_shared = false;
        else if (!have_shared) { have_shared = true; std::memcpy(g->shared_iw, di.inv + 9, 12); std::memcpy(g->shared_mw, di.m + 9, 12); }
        else if (std::memcmp(g->shared_iw, di.inv + 9, 12) != 0 || std::memcmp(g->shared_mw, di.m + 9, 12) != 0) all_shared = false;
        const bool emissive = scene.materials[inst.mat].type == MT_EMISSIVE;
        AreaTables areas;
        uint32_t light_index = ~0u;
        if (emissive) {
            areas = area_light_tables(mesh, inst.l2w);
            light_index = (uint32_t)g->lights.size();
            DevLight al{}; al.first_tri = (uint32_t)g->light_tris.size(); al.n_tris = mesh.n_tri; al.material = inst.mat; al.area_sum = areas.sum; al.kind = LK_AREA;
            g->lights.push_back(al);
        }
        lower_triangles(scene, (uint32_t)ii, l2r, di, emissive ? &areas : nullptr, light_index, g, &deg_render, &deg_local);
    }
    while (next_delta < delta.size()) lower_delta_light(delta[next_delta++], w2r, g);
    set_directional_areas(sb_lo, sb_hi, &g->lights);
    // which vertices will the traversal test?  (decided here, before the tree is built: mi355pt_scene_debug_set_lowering included)
    g->tris_are_local = all_shared && have_shared && scene.lowering < 1;
    filter_degenerate(g->tris_are_local ? deg_local : deg_render, g);
    if (g->build_tris.empty()) { *err = "scene has no triangles"; return MI355PT_E_INVALID; }
    if (g->build_tris.size() > ((size_t)MAX_LEAF_TRIS << MAX_BUILD_DEPTH)) { *err = "too many triangles"; return MI355PT_E_INVALID; }   // 16.7 M: depth bound of the traversal stack
    return MI355PT_OK;
}

// ---------------- a camera translation on a built scene (scene_rebase.cpp) ----------------

void mesh_local_bounds(const SceneImpl& scene, std::vector<MeshBounds>* out) {
    out->resize(scene.meshes.size());
    for (size_t i = 0; i < scene.meshes.size(); ++i) mesh_aabb(scene.meshes[i], (*out)[i].lo, (*out)[i].hi);
}

void mesh_local_bounds_of(const SceneImpl& scene, uint32_t geom, MeshBounds* out) { mesh_aabb(scene.meshes[geom], out->lo, out->hi); }

bool local_triangle_degenerate(const HostMesh& mesh, uint32_t tri) {
    return degenerate(vertex(mesh, mesh.idx[3 * tri]), vertex(mesh, mesh.idx[3 * tri + 1]), vertex(mesh, mesh.idx[3 * tri + 2]));
}

// lower_geometry's loop without its per-triangle work: the same functions in the same order on the same inputs
int lower_camera_records(const SceneImpl& scene, const mi355pt_camera* cam, const std::vector<MeshBounds>& bounds, const std::vector<DevLight>& built_lights,
                         const std::vector<DevLightTri>& built_light_tris, CameraRecords* out, std::string* err, const uint8_t* moved,
                         std::vector<float>* light_pdf) {
    const float w2r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -cam->position[0], -cam->position[1], -cam->position[2], 1};
    LoweredGeometry g;                                                         // the light list and the slots lower_delta_light fills
    g.env_light_index.assign(scene.envs.size(), 0u);
    g.env_l2r.resize(scene.envs.size());
    *out = CameraRecords{};
    out->instances.resize(scene.instances.size());
    out->light_tris = built_light_tris;                                        // cdf and pad stay; vertices and normal follow the camera
    bool all_shared = true, have_shared = false;
    float sb_lo[3] = {INFINITY, INFINITY, INFINITY}, sb_hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const std::vector<HostDeltaLight>& delta = scene.delta_lights;
    size_t next_delta = 0, lt = 0;
    if (light_pdf) light_pdf->assign(built_light_tris.size(), 0.0f);
    for (size_t ii = 0; ii < scene.instances.size(); ++ii) {
        while (next_delta < delta.size() && delta[next_delta].after_instances <= ii) lower_delta_light(delta[next_delta++], w2r, &g);
        const HostInstance& inst = scene.instances[ii];
        const HostMesh& mesh = scene.meshes[inst.geom];
        float l2r[16];
        mat4_mul(w2r, inst.l2w, l2r);
        grow_scene_bounds(bounds[inst.geom].lo, bounds[inst.geom].hi, l2r, sb_lo, sb_hi);
        DevInstance& di = out->instances[ii];
        if (!lower_transform(l2r, scene.lowering, inst.dynamic != 0u, &di)) { *err = "singular instance transform"; return MI355PT_E_INVALID; }
        if (!di.identity) all_shared = false;
        else if (!have_shared) { have_shared = true; std::memcpy(out->shared_iw, di.inv + 9, 12); std::memcpy(out->shared_mw, di.m + 9, 12); }
        else if (std::memcmp(out->shared_iw, di.inv + 9, 12) != 0 || std::memcmp(out->shared_mw, di.m + 9, 12) != 0) all_shared = false;
        if (scene.materials[inst.mat].type != MT_EMISSIVE) continue;
        // an area light's record holds world-space areas only (area_light_tables): it is the built one, unless the instance moved
        if (g.lights.size() >= built_lights.size() || lt + mesh.n_tri > out->light_tris.size()) { *err = "internal error: light list changed since the build"; return MI355PT_E_INVALID; }
        g.lights.push_back(built_lights[g.lights.size()]);
        if (moved && moved[ii]) {
            const AreaTables areas = area_light_tables(mesh, inst.l2w);
            g.lights.back().area_sum = areas.sum;
            for (uint32_t t = 0; t < mesh.n_tri; ++t) {
                out->light_tris[lt + t].cdf = areas.cdf[t];
                if (light_pdf) (*light_pdf)[lt + t] = light_pdf_area_of(areas.area, areas.cdf, t);
            }
        }
        for (uint32_t t = 0; t < mesh.n_tri; ++t, ++lt) {
            V3 p[3];
            for (int k = 0; k < 3; ++k) p[k] = xform_point(l2r, vertex(mesh, mesh.idx[3 * t + k]));
            DevLightTri& r = out->light_tris[lt];
            set_vertices(r, p[0], p[1], p[2]);
            const V3 n = normalize(normalize(cross(p[1] - p[0], p[2] - p[0])));
            r.n[0] = n.x; r.n[1] = n.y; r.n[2] = n.z;
        }
    }
    while (next_delta < delta.size()) lower_delta_light(delta[next_delta++], w2r, &g);
    if (g.lights.size() != built_lights.size() || lt != out->light_tris.size()) { *err = "internal error: light list changed since the build"; return MI355PT_E_INVALID; }
    set_directional_areas(sb_lo, sb_hi, &g.lights);
    out->lights = std::move(g.lights);
    out->env_light_index = std::move(g.env_light_index); out->env_l2r = std::move(g.env_l2r);
    out->tris_are_local = all_shared && have_shared && scene.lowering < 1;   // (a dynamic instance is never `shared`: its identity is 0)
    return MI355PT_OK;
}

// ---------------- new materials, lights and environments on a built scene (scene_edit.cpp) ----------------

void material_keys(const std::vector<DevMaterial>& materials, std::vector<EditMaterialKey>* out) {
    out->resize(materials.size());
    for (size_t i = 0; i < materials.size(); ++i) (*out)[i] = material_key(materials[i]);
}

// lower_scene's steps between pack_textures and the tree, on the description as it is now: the same functions in the same order
int lower_edit_records(const SceneImpl& scene, const mi355pt_camera* cam, const RebaseState& built, const uint8_t* material_changed, const uint8_t* env_edited,
                       EditRecords* out, std::string* err) {
    *out = EditRecords{};
    CameraRecords rec;
    if (int rc = lower_camera_records(scene, cam, built.bounds, built.lights, built.light_tris, &rec, err)) return rc;
    if (built.materials.size() != scene.materials.size() || built.envs.size() != scene.envs.size()) { *err = "internal error: material or environment list changed since the build"; return MI355PT_E_INVALID; }
    LoweredScene ls;
    ls.textures = built.textures;
    ls.materials = scene.materials;
    out->envs = built.envs;
    out->env_tables.resize(scene.envs.size());
    for (size_t ek = 0; ek < scene.envs.size(); ++ek) {
        const uint32_t li = rec.env_light_index[ek], hidden = rec.lights[li].material;
        if (!env_edited[ek]) { ls.materials[hidden] = built.materials[hidden]; continue; }        // the integrated spectrum the build computed
        if (int rc = lower_environment(scene, scene.envs[ek], rec.env_l2r[ek].data(), li, &out->env_tables[ek], &out->envs[ek], &ls.materials[hidden], err)) return rc;
    }
    const CoatRows reuse{built.materials, built.cc_albedo, material_changed};
    finish_materials(&ls, &reuse);
    out->materials = std::move(ls.materials);
    out->cc_albedo = std::move(ls.cc_albedo);
    out->lights = std::move(rec.lights);
    out->features = scene_features(scene, out->lights.size());
    return MI355PT_OK;
}

void keep_topology(const LoweredGeometry& geo, const BvhOut& bvh, const mi355pt_camera* cam, bool gpu_built, RebaseState* rb) {
    rb->gpu_built = gpu_built;
    std::memcpy(rb->tree_cam_pos, cam->position, sizeof(rb->tree_cam_pos));
    rb->tree_nodes = bvh.nodes; rb->tree_order = bvh.order; rb->tree_depth = bvh.max_depth; rb->tree_root = bvh.root;
    if (geo.n_degenerate) rb->kept = geo.kept;
    if (!geo.tris_are_local) {
        size_t k = 0;
        for (size_t t = 0; t < geo.tris.size(); ++t) {
            if (k < geo.kept.size() && geo.kept[k] == t) { ++k; continue; }
            rb->left_out.push_back(geo.shade[t].instance); rb->left_out.push_back(geo.shade[t].local_tri);
        }
    }
}

bool instance_transform_ok(const SceneImpl& scene, const mi355pt_camera* cam, const float* l2w) {
    for (int k = 0; k < 16; ++k) if (!std::isfinite(l2w[k])) return false;
    const float w2r[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -cam->position[0], -cam->position[1], -cam->position[2], 1};
    float l2r[16];
    mat4_mul(w2r, l2w, l2r);
    DevInstance di;
    return lower_transform(l2r, scene.lowering, false, &di);
}

bool render_triangle_degenerate(const SceneImpl& scene,const DevInstance& di, uint32_t instance, uint32_t tri) {
    const HostMesh& mesh = scene.meshes[scene.instances[instance].geom];
    const float l2r[16] = {di.m[0], di.m[1], di.m[2], 0, di.m[3], di.m[4], di.m[5], 0, di.m[6], di.m[7], di.m[8], 0, di.m[9], di.m[10], di.m[11], 1};
    V3 p[3];
    for (int k = 0; k < 3; ++k) p[k] = xform_point(l2r, vertex(mesh, mesh.idx[3 * tri + k]));
    return degenerate(p[0], p[1], p[2]);
}

bool same_lowering_class(const std::vector<DevInstance>& instances, bool tris_are_local, const std::vector<uint8_t>& identity, bool built_local) {
    if (tris_are_local != built_local || instances.size() != identity.size()) return false;
    for (size_t i = 0; i < instances.size(); ++i) if ((instances[i].identity != 0) != (identity[i] != 0)) return false;
    return true;
}

bool left_out_stay_degenerate(const SceneImpl& scene, const std::vector<DevInstance>& instances, const uint8_t* moved) {
    const std::vector<uint32_t>& lo = scene.rebase.left_out;
    for (size_t k = 0; k + 1 < lo.size(); k += 2)
        if ((!moved || moved[lo[k]]) && !render_triangle_degenerate(scene, instances[lo[k]], lo[k], lo[k + 1])) return false;
    return true;
}

int lower_scene(const SceneImpl& scene, LoweredGeometry&& g, BvhOut&& bvh, const float* cmf4, LoweredScene* ls, LowerReport* rep, std::string* err) {
    *ls = LoweredScene{};
    reorder_to_leaves(g, bvh.order, ls);
    pack_spectral_tables(scene, cmf4, ls);
    pack_textures(scene, ls);
    ls->materials = scene.materials;
    ls->env_tables.resize(scene.envs.size());
    ls->envs.resize(scene.envs.size());
    for (size_t ek = 0; ek < scene.envs.size(); ++ek) {
        const uint32_t li = g.env_light_index[ek];
        if (int rc = lower_environment(scene, scene.envs[ek], g.env_l2r[ek].data(), li, &ls->env_tables[ek], &ls->envs[ek], &ls->materials[g.lights[li].material], err)) return rc;
    }
    finish_materials(ls);
    ls->nodes = std::move(bvh.nodes);
    ls->instances = std::move(g.instances);
    ls->lights = std::move(g.lights);
    ls->light_tris = std::move(g.light_tris);
    ls->light_uvs = std::move(g.light_uvs);
    ls->features = scene_features(scene, ls->lights.size());
    DevScene& dev = ls->dev;
    dev.tris_are_local = g.tris_are_local ? 1u : 0u;                          // (lowering >= 1, mi355pt_scene_debug_set_lowering: never)
    for (int k = 0; k < 3; ++k) { dev.tri_shift[k] = g.tris_are_local ? g.shared_iw[k] : 0.0f; dev.shared_mw[k] = g.tris_are_local ? g.shared_mw[k] : 0.0f; }
    dev.n_envs = (uint32_t)ls->envs.size();
    dev.n_nodes = (uint32_t)ls->nodes.size(); dev.n_tris = (uint32_t)ls->tris_render.size();
    dev.n_lights = (uint32_t)ls->lights.size(); dev.n_materials = (uint32_t)ls->materials.size();
    dev.root = bvh.root;
    rep->n_degenerate = g.n_degenerate;
    rep->bvh_depth = bvh.max_depth;
    return MI355PT_OK;
}

int lower_tree4(LoweredScene* ls, LowerReport* rep, std::string* err) {
    std::vector<DevNode4> nodes4;
    if (!collapse_bvh4(ls->nodes, ls->dev.root, ls->tris_render.size(), &nodes4, &ls->dev.root4, &rep->stack_need, err, &rep->collapse_method)) return MI355PT_E_INVALID;
    ls->dev.n_nodes4 = (uint32_t)nodes4.size();
#if PT_NODE_FMA
    pad_nodes4(&nodes4);
#endif
#if PT_NODE_Q16
    if (!quantise_nodes4(nodes4, ls->dev.grid_org, ls->dev.grid_cell, &ls->nodes4, err)) return MI355PT_E_INVALID;
#else
    ls->nodes4 = std::move(nodes4);
#endif
    return MI355PT_OK;
}

std::string lowering_info(const LoweredScene& ls, const LowerReport& rep, bool gpu_builder, const double* ms) {
    char t_bvh[64] = "", t_collapse[32] = "", tail[160];
    if (ms) { std::snprintf(t_bvh, sizeof(t_bvh), " bvh_ms=%.2f bvh_device_ms=%.2f", ms[0], ms[1]); std::snprintf(t_collapse, sizeof(t_collapse), " collapse_ms=%.2f", ms[2]); }
    std::snprintf(tail, sizeof(tail), " stack_need=%d/%d degenerate=%zu tri_space=%s features=%u", rep.stack_need, STACK_DEPTH, rep.n_degenerate,
                  ls.dev.tris_are_local ? "local" : "render", ls.features);
    return "nodes4=" + std::to_string(ls.dev.n_nodes4) + " nodes=" + std::to_string(ls.nodes.size()) + " tris=" + std::to_string(ls.tris_render.size()) +
           " depth=" + std::to_string(rep.bvh_depth) + " builder=" + (gpu_builder ? "gpu" : "host") + t_bvh + " collapse=" + rep.collapse_method + t_collapse + tail;
}

void lowering_digests(const LoweredScene& ls, const LowerReport& rep, std::vector<std::string>* names, std::vector<uint64_t>* digests) {
    names->clear(); digests->clear();
    auto add = [&](const std::string& name, const void* p, size_t bytes) { names->push_back(name); digests->push_back(fnv1a64(p, bytes)); };
#define PT_DIGEST(v) add(#v, ls.v.data(), ls.v.size() * sizeof(ls.v[0]))
    PT_DIGEST(nodes); PT_DIGEST(nodes4); PT_DIGEST(tris_render); PT_DIGEST(shade); PT_DIGEST(instances); PT_DIGEST(tris_local); PT_DIGEST(cc_albedo);
    PT_DIGEST(materials); PT_DIGEST(lights); PT_DIGEST(light_tris); PT_DIGEST(light_uvs); PT_DIGEST(luts); PT_DIGEST(cmf); PT_DIGEST(rgb2spec);
    PT_DIGEST(z_nodes); PT_DIGEST(texels); PT_DIGEST(textures);
#undef PT_DIGEST
    for (size_t k = 0; k < ls.env_tables.size(); ++k) {
        const LoweredScene::EnvTables& t = ls.env_tables[k];
        const std::string e = "env" + std::to_string(k);
        add(e + ".texels", t.texels.data(), t.texels.size() * 4); add(e + ".marginal", t.marginal.data(), t.marginal.size() * 4);
        add(e + ".conditional", t.conditional.data(), t.conditional.size() * 4);
    }
    add("envs", ls.envs.data(), ls.envs.size() * sizeof(DevEnv));           // (their pointers are null before the upload)
    std::string b;                                                          // the scalars, field by field in DevScene's order, then features and the report
    auto put = [&](const void* p, size_t n) { b.append((const char*)p, n); };
    const DevScene& dev = ls.dev;
    put(dev.grid_org, 12); put(dev.grid_cell, 12); put(dev.tri_shift, 12); put(&dev.tris_are_local, 4); put(dev.shared_mw, 12); put(&dev.pad_mw, 4);
    put(&dev.n_nodes, 4); put(&dev.n_tris, 4); put(&dev.n_lights, 4); put(&dev.n_materials, 4); put(&dev.root, 4); put(&dev.root4, 4);
    put(&dev.n_nodes4, 4); put(&dev.cam_lists, 4); put(&dev.n_envs, 4); put(&dev.queue_stage, 2); put(&dev.light_queue, 1); put(&dev.early_path_end, 1);
    const uint32_t feat = ls.features; const uint64_t ndeg = rep.n_degenerate, nn4 = dev.n_nodes4; const int32_t depth = rep.bvh_depth, need = rep.stack_need;
    put(&feat, 4); put(&ndeg, 8); put(&depth, 4); put(&nn4, 8); put(&need, 4); put(rep.collapse_method, std::strlen(rep.collapse_method));
    add("scalars", b.data(), b.size());
}

}  // namespace pt
