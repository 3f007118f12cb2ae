// The debug surface of the in-place scene updates (include/mi355pt_debug.h): the two pinned lowerings the tests hold the three updates to, their digests and exports, the host-only
// pin and instance transform, the host SAH sum, the read-back digest of the device arrays.  Host C++ only; mi355pt_scene_debug_set_mesh_vertices is scene_deform.cpp's (it shares its checks).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "api_internal.hpp"
#include "instance_move_plan.hpp"
#include "rebase_plan.hpp"
#include "scene_lower.hpp"

using namespace pt;

namespace {

int digests_out(const LoweredScene& ls, const LowerReport& rep, bool gpu_builder, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n) {
    std::vector<std::string> names; std::vector<uint64_t> dig;
    lowering_digests(ls, rep, &names, &dig);
    std::string text;
    for (const std::string& nm : names) text += nm + "\n";
    text += lowering_info(ls, rep, gpu_builder, nullptr);
    const uint32_t cap = *n;
    *n = (uint32_t)dig.size();
    if (cap < dig.size() || names_len < text.size() + 1) return fail(MI355PT_E_INVALID, "digest or name buffer too small");
    std::memcpy(digests, dig.data(), dig.size() * sizeof(uint64_t));
    std::memcpy(names_buf, text.c_str(), text.size() + 1);
    return MI355PT_OK;
}

// mi355pt_scene_debug_move_digest's lowering: *ls / *rep for cam_new over the tree of cam_built (or a fresh lowering where a move rebuilds)
int pinned_lowering(const mi355pt_scene* s, const mi355pt_camera* cam_built, const mi355pt_camera* cam_new, LoweredScene* ls_out, LowerReport* rep_out,
                    uint32_t* out_reason, bool* out_gpu_tree, float* out_radii /* 2: the root record's, pad_nodes4's own; NULL ok */) {
#if PT_NODE_Q16
    return fail(MI355PT_E_INVALID, "a build with quantised 4-wide nodes does not re-base");
#else
    const SceneImpl& impl = s->impl;
    std::string err;
    int rc;
    float cmf[470 * 4];
    cie_cmf4(cmf);
    // the lowering for cam_built: its tree is the topology everything below is pinned to.  A scene whose tree WAS built at cam_built by the GPU
    // builder pins to that tree, which the build kept on the host; every other tree is the host builder's
    LoweredGeometry geo_b; BvhOut bvh_b; LoweredScene ls_b; LowerReport rep_b;
    if ((rc = lower_geometry(impl, cam_built, &geo_b, &err))) return fail(rc, err);
    const bool gpu_tree = impl.built && impl.rebase.gpu_built && std::memcmp(cam_built->position, impl.rebase.tree_cam_pos, sizeof(float) * 3) == 0 &&
                          impl.rebase.tree_order.size() == geo_b.build_tris.size();
    if (gpu_tree) { bvh_b.nodes = impl.rebase.tree_nodes; bvh_b.order = impl.rebase.tree_order; bvh_b.root = impl.rebase.tree_root; bvh_b.max_depth = impl.rebase.tree_depth; }
    else build_bvh(geo_b.build_tris, &bvh_b);
    if (bvh_b.max_depth >= STACK_DEPTH) return fail(MI355PT_E_INVALID, "BVH deeper than the traversal stack");
    const BvhOut topology = bvh_b;
    const std::vector<uint32_t> kept_b = geo_b.kept;
    std::vector<uint8_t> identity_b(geo_b.instances.size());
    for (size_t i = 0; i < identity_b.size(); ++i) identity_b[i] = (uint8_t)geo_b.instances[i].identity;
    const bool local_b = geo_b.tris_are_local;
    if ((rc = lower_scene(impl, std::move(geo_b), std::move(bvh_b), cmf, &ls_b, &rep_b, &err)) || (rc = lower_tree4(&ls_b, &rep_b, &err))) return fail(rc, err);

    LoweredGeometry geo_n;
    if ((rc = lower_geometry(impl, cam_new, &geo_n, &err))) return fail(rc, err);
    uint32_t reason = std::memcmp(cam_built->position, cam_new->position, sizeof(float) * 3) == 0 ? MI355PT_MOVE_SAME_POSITION : MI355PT_MOVE_REBASED;
    if (!same_lowering_class(geo_n.instances, geo_n.tris_are_local, identity_b, local_b)) reason = MI355PT_MOVE_INSTANCE_CLASS_CHANGED;
    else if (geo_n.kept != kept_b) reason = MI355PT_MOVE_DEGENERATE_SET_CHANGED;
    if (out_reason) *out_reason = reason;
    LoweredScene& ls_n = *ls_out; LowerReport& rep_n = *rep_out;
    const bool rebuilds = reason == MI355PT_MOVE_INSTANCE_CLASS_CHANGED || reason == MI355PT_MOVE_DEGENERATE_SET_CHANGED;
    *out_gpu_tree = gpu_tree && !rebuilds;
    if (rebuilds) {
        // the move builds again: what a fresh lowering gives (the host builder's tree)
        BvhOut bvh_n;
        build_bvh(geo_n.build_tris, &bvh_n);
        if (bvh_n.max_depth >= STACK_DEPTH) return fail(MI355PT_E_INVALID, "BVH deeper than the traversal stack");
        if ((rc = lower_scene(impl, std::move(geo_n), std::move(bvh_n), cmf, &ls_n, &rep_n, &err)) || (rc = lower_tree4(&ls_n, &rep_n, &err))) return fail(rc, err);
    } else {
        // the new geometry in the old tree: stage B with cam_built's links and leaf order, then every box from the new triangles
        RebasePlan plan;
        if (!make_rebase_plan(ls_b.nodes, ls_b.dev.root, ls_b.nodes4, ls_b.dev.root4, ls_b.tris_render.size(), &plan)) return fail(MI355PT_E_INVALID, "internal error: no refit plan for the built tree");
        BvhOut pinned = topology;
        if ((rc = lower_scene(impl, std::move(geo_n), std::move(pinned), cmf, &ls_n, &rep_n, &err))) return fail(rc, err);
        ls_n.nodes4 = ls_b.nodes4;                                   // cam_built's collapse: links, used slots; the boxes follow
        ls_n.dev.root4 = ls_b.dev.root4; ls_n.dev.n_nodes4 = ls_b.dev.n_nodes4;
        rep_n.stack_need = rep_b.stack_need; rep_n.collapse_method = rep_b.collapse_method;
        refit_host(plan, ls_n.dev.root, ls_n.tris_render.data(), &ls_n.nodes, &ls_n.nodes4);
    }
    if (out_radii) {
        // the pad's r two ways: from the root record (what the device computes) and by pad_nodes4's own loop over the UNPADDED 4-wide boxes,
        // i.e. the BVH2 boxes its slots carry
        RebasePlan plan;
        if (!make_rebase_plan(ls_n.nodes, ls_n.dev.root, ls_n.nodes4, ls_n.dev.root4, ls_n.tris_render.size(), &plan)) return fail(MI355PT_E_INVALID, "internal error: no refit plan");
        std::vector<DevNode4> bare = ls_n.nodes4;
        for (size_t i = 0; i < plan.slot_src.size(); ++i) if (plan.slot_src[i] != REBASE_NO_SOURCE) store_slot_box(bare[i >> 2], (int)(i & 3u), ls_n.nodes[plan.slot_src[i] >> 1], (int)(plan.slot_src[i] & 1u), 0.0f);
        out_radii[0] = ls_n.dev.root >= 0 ? pad_radius(ls_n.nodes[(size_t)ls_n.dev.root]) : 0.0f;
        out_radii[1] = nodes4_pad_radius(bare);
    }
    return MI355PT_OK;
#endif
}

// mi355pt_scene_debug_pinned_digest's lowering: the CURRENT description for `cam` over the topology the built scene holds (the build keeps
// both trees on the host), every box refit from the new triangles
int pinned_current(const mi355pt_scene* s, const mi355pt_camera* cam, LoweredScene* ls, LowerReport* rep) {
#if PT_NODE_Q16
    return fail(MI355PT_E_INVALID, "a build with quantised 4-wide nodes does not re-base");
#else
    const SceneImpl& impl = s->impl;
    const RebaseState& rb = impl.rebase;
    if (!impl.built && !rb.pinned) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (!rb.pinned) return fail(MI355PT_E_INVALID, "the built tree has no refit plan");
    std::string err;
    int rc;
    float cmf[470 * 4];
    cie_cmf4(cmf);
    LoweredGeometry geo;
    if ((rc = lower_geometry(impl, cam, &geo, &err))) return fail(rc, err);
    bool same = geo.kept.size() == rb.tree_order.size() && geo.n_degenerate == rb.n_degenerate && same_lowering_class(geo.instances, geo.tris_are_local, rb.identity, rb.tris_are_local);
    if (same && geo.n_degenerate) same = geo.kept == rb.kept;
    if (!same) return fail(MI355PT_E_INVALID, "the description no longer lowers over the built tree (degenerate set or instance class changed)");
    RebasePlan plan;
    if (!make_rebase_plan(rb.tree_nodes, rb.tree_root, rb.tree_nodes4, rb.tree_root4, rb.tree_order.size(), &plan)) return fail(MI355PT_E_INVALID, "internal error: no refit plan for the built tree");
    BvhOut pinned;
    pinned.nodes = rb.tree_nodes; pinned.order = rb.tree_order; pinned.root = rb.tree_root; pinned.max_depth = rb.tree_depth;
    if ((rc = lower_scene(impl, std::move(geo), std::move(pinned), cmf, ls, rep, &err))) return fail(rc, err);
    ls->nodes4 = rb.tree_nodes4;
    ls->dev.root4 = rb.tree_root4; ls->dev.n_nodes4 = (uint32_t)rb.tree_nodes4.size();
    rep->stack_need = rb.stack_need; rep->collapse_method = rb.collapse_method.c_str();
    refit_host(plan, ls->dev.root, ls->tris_render.data(), &ls->nodes, &ls->nodes4);
    return MI355PT_OK;
#endif
}

// the exports' common part: nodes, triangles and root out; a buffer that is given holds *n_nodes / *n_tris records, which receive the counts
int export_out(const LoweredScene& ls, void* out_nodes, uint32_t* n_nodes, void* out_tris, uint32_t* n_tris, int32_t* root) {
    if (out_nodes) { if (*n_nodes < ls.nodes.size()) return fail(MI355PT_E_INVALID, "node buffer too small"); std::memcpy(out_nodes, ls.nodes.data(), ls.nodes.size() * sizeof(DevNode)); }
    if (out_tris) { if (*n_tris < ls.tris_render.size()) return fail(MI355PT_E_INVALID, "triangle buffer too small"); std::memcpy(out_tris, ls.tris_render.data(), ls.tris_render.size() * sizeof(DevTri)); }
    *n_nodes = (uint32_t)ls.nodes.size(); *n_tris = (uint32_t)ls.tris_render.size();
    if (root) *root = ls.dev.root;
    return MI355PT_OK;
}

}  // namespace

extern "C" {

int mi355pt_scene_debug_move_digest(const mi355pt_scene* s, const mi355pt_camera* cam_built, const mi355pt_camera* cam_new, char* names_buf, size_t names_len,
                                    uint64_t* digests, uint32_t* n, uint32_t* out_reason) {
    if (!s || !cam_built || !cam_new || !names_buf || !digests || !n) return fail(MI355PT_E_INVALID, "null argument");
    LoweredScene ls; LowerReport rep; bool gpu_tree = false;
    if (int rc = pinned_lowering(s, cam_built, cam_new, &ls, &rep, out_reason, &gpu_tree, nullptr)) return rc;
    return digests_out(ls, rep, gpu_tree, names_buf, names_len, digests, n);
}

int mi355pt_scene_debug_move_export(const mi355pt_scene* s, const mi355pt_camera* cam_built, const mi355pt_camera* cam_new, void* out_nodes, uint32_t* n_nodes,
                                    void* out_tris, uint32_t* n_tris, int32_t* root, float* out_pad_radii) {
    if (!s || !cam_built || !cam_new || !n_nodes || !n_tris) return fail(MI355PT_E_INVALID, "null argument");
    LoweredScene ls; LowerReport rep; bool gpu_tree = false;
    if (int rc = pinned_lowering(s, cam_built, cam_new, &ls, &rep, nullptr, &gpu_tree, out_pad_radii)) return rc;
    return export_out(ls, out_nodes, n_nodes, out_tris, n_tris, root);
}

int mi355pt_scene_debug_pinned_digest(const mi355pt_scene* s, const mi355pt_camera* cam, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n) {
    if (!s || !cam || !names_buf || !digests || !n) return fail(MI355PT_E_INVALID, "null argument");
    LoweredScene ls; LowerReport rep;
    if (int rc = pinned_current(s, cam, &ls, &rep)) return rc;
    return digests_out(ls, rep, s->impl.rebase.gpu_built, names_buf, names_len, digests, n);
}

int mi355pt_scene_debug_pinned_export(const mi355pt_scene* s, const mi355pt_camera* cam, void* out_nodes, uint32_t* n_nodes, void* out_tris, uint32_t* n_tris,
                                      int32_t* root, uint32_t* out_entries, uint32_t* n_entries) {
    if (!s || !cam || !n_nodes || !n_tris) return fail(MI355PT_E_INVALID, "null argument");
    LoweredScene ls; LowerReport rep;
    if (int rc = pinned_current(s, cam, &ls, &rep)) return rc;
    if (int rc = export_out(ls, out_nodes, n_nodes, out_tris, n_tris, root)) return rc;
#if !PT_NODE_Q16
    if (n_entries) {
        RebasePlan plan;
        if (!make_rebase_plan(ls.nodes, ls.dev.root, ls.nodes4, ls.dev.root4, ls.tris_render.size(), &plan)) return fail(MI355PT_E_INVALID, "internal error: no refit plan");
        if (out_entries) { if (*n_entries < plan.entries.size()) return fail(MI355PT_E_INVALID, "entry buffer too small"); std::memcpy(out_entries, plan.entries.data(), plan.entries.size() * sizeof(uint32_t)); }
        *n_entries = (uint32_t)plan.entries.size();
    }
#endif
    return MI355PT_OK;
}

int mi355pt_scene_debug_pin_host_tree(mi355pt_scene* s, const mi355pt_camera* cam) {
    if (!s || !cam) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& impl = s->impl;
    if (impl.built || !s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_debug_pin_host_tree is for a scene that is not built");
    impl.rebase = RebaseState{};
    std::string err;
    int rc;
    float cmf[470 * 4];
    cie_cmf4(cmf);
    LoweredGeometry geo; BvhOut bvh; LoweredScene ls; LowerReport rep;
    if ((rc = lower_geometry(impl, cam, &geo, &err))) return fail(rc, err);
    build_bvh(geo.build_tris, &bvh);
    if (bvh.max_depth >= STACK_DEPTH) return fail(MI355PT_E_INVALID, "BVH deeper than the traversal stack");
    keep_topology(geo, bvh, cam, false, &impl.rebase);
    if ((rc = lower_scene(impl, std::move(geo), std::move(bvh), cmf, &ls, &rep, &err)) || (rc = lower_tree4(&ls, &rep, &err)) ||
        (rc = impl.prepare_rebase(ls, rep, &err, false))) return fail(rc, err);
    if (!impl.rebase.pinned) return fail(MI355PT_E_INVALID, "the tree has no refit plan");
    std::memcpy(impl.build_cam_pos, cam->position, sizeof(impl.build_cam_pos));
    return MI355PT_OK;
}

int mi355pt_scene_debug_set_instance_transform(mi355pt_scene* s, uint32_t instance, const float* local_to_world) {
    if (!s || !local_to_world) return fail(MI355PT_E_INVALID, "null argument");
    if (s->impl.built || !s->parts.empty()) return fail(MI355PT_E_INVALID, "a built scene moves with mi355pt_scene_move_instances");
    if (instance >= s->impl.instances.size()) return fail(MI355PT_E_INVALID, "bad instance id");
    std::memcpy(s->impl.instances[instance].l2w, local_to_world, sizeof(float) * 16);
    return MI355PT_OK;
}

int mi355pt_debug_sah_cost(const void* nodes, uint32_t n_nodes, int32_t root, const uint32_t* entries, uint32_t n_entries, float* out_cost) {
    if ((!nodes && n_nodes) || (!entries && n_entries) || !out_cost) return fail(MI355PT_E_INVALID, "null argument");
    for (uint32_t k = 0; k < n_entries; ++k) if ((entries[k] >> 1) >= n_nodes) return fail(MI355PT_E_INVALID, "entry names a node out of range");
    if (root >= 0 && (uint32_t)root >= n_nodes) return fail(MI355PT_E_INVALID, "root out of range");
    const DevNode* p = (const DevNode*)nodes;
    *out_cost = sah_cost_host(std::vector<DevNode>(p, p + n_nodes), root, std::vector<uint32_t>(entries, entries + n_entries));
    return MI355PT_OK;
}

int mi355pt_scene_debug_device_digest(const mi355pt_scene* s, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n) {
    if (!s || !names_buf || !digests || !n) return fail(MI355PT_E_INVALID, "null argument");
    const SceneImpl& impl = s->impl;
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    HIP_TRY(hipDeviceSynchronize());
    const DevScene& d = impl.dev;
    LoweredScene ls;
    // SceneImpl::upload's order is the order of SceneImpl::allocs; every array's length is known from the scene record or the description
#define PT_READ(vec, ptr, count)                                                                                                       \
    do {                                                                                                                               \
        ls.vec.resize(count);                                                                                                          \
        if (!ls.vec.empty()) HIP_TRY(hipMemcpy(ls.vec.data(), (const void*)(ptr), ls.vec.size() * sizeof(ls.vec[0]), hipMemcpyDeviceToHost)); \
    } while (0)
    size_t n_light_tris = 0, n_luts = 0, n_texels = 0, n_cc = 0;
    PT_READ(nodes, d.nodes, d.n_nodes);
#if PT_NODE_Q16
    PT_READ(nodes4, d.nodes4q, d.n_nodes4);
#else
    PT_READ(nodes4, d.nodes4, d.n_nodes4);
#endif
    PT_READ(tris_render, d.tris_render, d.n_tris);
    PT_READ(shade, d.shade, d.n_tris);
    PT_READ(instances, d.instances, impl.instances.size());
    PT_READ(tris_local, d.tris_local, d.n_tris);
    PT_READ(materials, d.materials, d.n_materials);
    for (const DevMaterial& m : ls.materials) if (m.type == MT_CLEARCOAT) ++n_cc;
    PT_READ(cc_albedo, d.cc_albedo, std::max<size_t>(n_cc, 1) * 64);
    PT_READ(lights, d.lights, d.n_lights);
    for (const DevLight& l : ls.lights) if (l.kind == LK_AREA) n_light_tris += l.n_tris;
    PT_READ(light_tris, d.light_tris, n_light_tris);
    PT_READ(light_uvs, d.light_uvs, n_light_tris * 6);
    for (const std::vector<float>& l : impl.luts) n_luts += l.size();
    PT_READ(luts, d.luts, n_luts);
    PT_READ(cmf, d.cmf, (size_t)470 * 4);
    PT_READ(rgb2spec, d.rgb2spec, impl.table.empty() ? (size_t)0 : (size_t)3 * 64 * 64 * 64 * 4);
    PT_READ(z_nodes, d.z_nodes, impl.table.empty() ? (size_t)0 : (size_t)64);
    for (const SceneImpl::Tex& t : impl.textures) n_texels += (size_t)t.w * t.h;
    PT_READ(texels, d.texels, n_texels);
    PT_READ(textures, d.textures, impl.textures.size());
    PT_READ(envs, d.envs, d.n_envs);
    ls.env_tables.resize(ls.envs.size());
    for (size_t k = 0; k < ls.envs.size(); ++k) {
        DevEnv& e = ls.envs[k];
        const size_t px = (size_t)e.w * e.h;
        PT_READ(env_tables[k].texels, e.texels, px * 4);
        PT_READ(env_tables[k].marginal, e.marginal, (size_t)e.h);
        PT_READ(env_tables[k].conditional, e.conditional, px);
        e.texels = e.marginal = e.conditional = nullptr;              // pointers count as null, as in the lowering digest
    }
#undef PT_READ
    ls.dev = d;
    ls.features = impl.features;
    LowerReport rep;
    rep.n_degenerate = impl.rebase.n_degenerate; rep.bvh_depth = impl.rebase.bvh_depth; rep.stack_need = impl.rebase.stack_need;
    rep.collapse_method = impl.rebase.collapse_method.c_str();
    return digests_out(ls, rep, impl.rebase.gpu_built, names_buf, names_len, digests, n);
}

}  // extern "C"
