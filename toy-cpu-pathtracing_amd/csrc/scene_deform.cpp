// Deforming meshes of a built scene (include/mi355pt_deform.h): the call itself and its host-only twin of the debug surface.  Host C++
// only; the device half is scene_update.cpp's step, the kernel is pt_kernels_deform.hip, the rest of the move the instance move's launches
// (pt_kernels_rebase.hip, pt_kernels_instances.hip); the layout host and device share is deform_plan.hpp.  The side tables are
// RebaseState's (scene.hpp); the host form the tests hold the deformation to is mi355pt_scene_debug_pinned_digest (scene_debug.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "scene_update.hpp"

using namespace pt;

namespace {

// one update, checked: the arrays as the description will hold them
struct Checked {
    uint32_t geom = 0;
    const float* pos = nullptr;
    std::vector<float> nrm;                 // normalised like mi355pt_scene_add_mesh's; empty = keep
    const float* tangent = nullptr;         // null = keep
    bool changed = false;                   // some array differs bytewise from the description's
};

// every check of the arguments that needs no device and no built scene; *err names the first one that fails
bool check_updates(const SceneImpl& impl, const mi355pt_mesh_update* updates, uint32_t n, std::vector<Checked>* out, std::string* err) {
    out->clear();
    for (uint32_t k = 0; k < n; ++k) {
        const mi355pt_mesh_update& u = updates[k];
        if (u.geom >= impl.meshes.size()) { *err = "bad geom id"; return false; }
        if (k && u.geom <= updates[k - 1].geom) { *err = "geom ids must be strictly ascending"; return false; }
        if (!u.pos) { *err = "null vertex positions"; return false; }
        const HostMesh& m = impl.meshes[u.geom];
        if (u.tri_tangent && m.uv.empty()) { *err = "tri_tangent given for a mesh without uv"; return false; }
        for (size_t i = 0; i < (size_t)m.n_vert * 3; ++i) if (!std::isfinite(u.pos[i])) { *err = "non-finite vertex position"; return false; }
    }
    out->resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        const mi355pt_mesh_update& u = updates[k];
        const HostMesh& m = impl.meshes[u.geom];
        Checked& c = (*out)[k];
        c.geom = u.geom; c.pos = u.pos; c.tangent = u.tri_tangent;
        if (u.nrm) {
            c.nrm.resize((size_t)m.n_vert * 3);
            for (uint32_t i = 0; i < m.n_vert; ++i) {   // Normal::new normalises and Normal::from renormalises (api_scene.cpp mi355pt_scene_add_mesh)
                const V3 v = norm3(norm3(V3{u.nrm[3 * i], u.nrm[3 * i + 1], u.nrm[3 * i + 2]}));
                c.nrm[3 * i] = v.x; c.nrm[3 * i + 1] = v.y; c.nrm[3 * i + 2] = v.z;
            }
        }
        c.changed = !deform_same_bytes(c.pos, m.pos.data(), m.pos.size()) || !deform_same_bytes(c.nrm.empty() ? nullptr : c.nrm.data(), m.nrm.data(), m.nrm.size()) ||
                    !deform_same_bytes(c.tangent, m.tangent.data(), m.tangent.size());
    }
    return true;
}

// the description takes the new arrays (counts and indices stay), and the cached local boxes follow where a build or a pin made them
void apply_updates(SceneImpl* impl, const std::vector<Checked>& ups) {
    for (const Checked& c : ups) {
        if (!c.changed) continue;
        HostMesh& m = impl->meshes[c.geom];
        m.pos.assign(c.pos, c.pos + m.pos.size());
        if (!c.nrm.empty()) m.nrm = c.nrm;
        if (c.tangent) m.tangent.assign(c.tangent, c.tangent + m.tangent.size());
        if (c.geom < impl->rebase.bounds.size()) mesh_local_bounds_of(*impl, c.geom, &impl->rebase.bounds[c.geom]);
    }
}

}  // namespace

extern "C" {

int mi355pt_scene_deform_meshes(mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_mesh_update* updates, uint32_t n, const mi355pt_instance_move_params* p,
                                mi355pt_instance_move_result* out) {
    const auto t0 = std::chrono::steady_clock::now();
    mi355pt_instance_move_result r{};
    if (out) *out = r;
    if (!s || !cam || !updates || n == 0) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& impl = s->impl;
    std::vector<Checked> ups;
    std::string err;
    if (!check_updates(impl, updates, n, &ups, &err)) return fail(MI355PT_E_INVALID, err);
    const float rebuild_above = p ? p->rebuild_above : 0.0f;
    if (p && !(rebuild_above >= 0.0f)) return fail(MI355PT_E_INVALID, "rebuild_above must be 0 or positive");
    if (!s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_deform_meshes does not deform a scene built with mi355pt_scene_build_multi: build it again");
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (std::memcmp(cam->position, impl.build_cam_pos, sizeof(float) * 3) != 0) return fail(MI355PT_E_INVALID, "camera position differs from the position the scene is at: call mi355pt_scene_move_camera first");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    auto done = [&](int rc) { r.host_ms = ms_since(t0); if (out) *out = r; return rc; };

    std::vector<DeformUpdate> changed;
    std::vector<const Checked*> changed_src;
    for (const Checked& c : ups)
        if (c.changed) { changed.push_back(DeformUpdate{c.geom, impl.meshes[c.geom].n_vert, impl.meshes[c.geom].n_tri, !c.nrm.empty(), c.tangent != nullptr}); changed_src.push_back(&c); }
    if (changed.empty()) { r.reason = MI355PT_MOVE_SAME_VERTICES; return done(MI355PT_OK); }

    RebaseState& rb = impl.rebase;
    // local-triangle mode decides "degenerate" on the LOCAL vertices (lower_geometry: deg_local): the set as it is before the description changes
    std::vector<std::vector<uint8_t>> deg_before(changed.size());
    if (rb.ready && rb.tris_are_local)
        for (size_t k = 0; k < changed.size(); ++k) {
            const HostMesh& m = impl.meshes[changed[k].geom];
            deg_before[k].resize(m.n_tri);
            for (uint32_t t = 0; t < m.n_tri; ++t) deg_before[k][t] = local_triangle_degenerate(m, t) ? 1 : 0;
        }
    // the description takes the new arrays now: everything below — the records, the checks, a rebuild — is computed from it
    apply_updates(&impl, ups);
    auto rebuild = [&](uint32_t reason) { r.rebuilt = 1; r.reason = reason; r.launches = 0; r.device_ms = 0.0; r.sah_built = r.sah_after = 0.0f; return done(mi355pt_scene_build(s, cam)); };
    if (!rb.ready) return rebuild(MI355PT_MOVE_UNSUPPORTED_BUILD);

    // host: the layout of this call, the small records with the lowering's own functions, the deformed area lights' tables; then the cases
    // in which a deformation in place is not what a fresh lowering gives
    std::vector<uint32_t> instance_geom(impl.instances.size()), mesh_n_vert(impl.meshes.size()), mesh_n_tri(impl.meshes.size());
    for (size_t i = 0; i < impl.instances.size(); ++i) instance_geom[i] = impl.instances[i].geom;
    for (size_t g = 0; g < impl.meshes.size(); ++g) { mesh_n_vert[g] = impl.meshes[g].n_vert; mesh_n_tri[g] = impl.meshes[g].n_tri; }
    if (rb.mesh_idx_offset.empty()) { rb.mesh_idx_offset = deform_index_offsets(mesh_n_tri.data(), mesh_n_tri.size()); rb.mesh_idx_uploaded.assign(impl.meshes.size(), 0); }
    DeformPlan plan;
    if (!make_deform_plan(instance_geom.data(), instance_geom.size(), mesh_n_vert.data(), mesh_n_tri.data(), mesh_n_tri.size(), rb.mesh_idx_offset, changed.data(), changed.size(), &plan))
        return done(fail(MI355PT_E_INVALID, "internal error: no deformation plan"));
    CameraRecords rec;
    std::vector<float> light_pdf;
    if (int rc = lower_camera_records(impl, cam, rb.bounds, rb.lights, rb.light_tris, &rec, &err, plan.moved.data(), &light_pdf)) return done(fail(rc, err));
    // (no matrix changed, so the classes of the lowering — DevInstance::identity, tris_are_local — are the build's: nothing to compare)
    if (!left_out_stay_degenerate(impl, rec.instances, plan.moved.data())) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);   // a triangle the tree leaves out may no longer be degenerate (render space)
    if (rb.tris_are_local)                                        // ... and the local-space set, either way
        for (size_t k = 0; k < changed.size(); ++k) {
            const HostMesh& m = impl.meshes[changed[k].geom];
            for (uint32_t t = 0; t < m.n_tri; ++t) if ((local_triangle_degenerate(m, t) ? 1 : 0) != deg_before[k][t]) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);
        }

    // the staging buffer in the plan's layout
    std::vector<float> staging(plan.staging_floats);
    for (size_t k = 0; k < changed.size(); ++k) {
        const Checked& c = *changed_src[k];
        const DeformSlot& sl = plan.slots[k];
        std::memcpy(staging.data() + sl.pos, c.pos, (size_t)3 * sl.n_vert * sizeof(float));
        if (sl.nrm != DEFORM_NO_SLOT) std::memcpy(staging.data() + sl.nrm, c.nrm.data(), (size_t)3 * sl.n_vert * sizeof(float));
        if (sl.tangent != DEFORM_NO_SLOT) std::memcpy(staging.data() + sl.tangent, c.tangent, (size_t)3 * sl.n_tri * sizeof(float));
    }
    const std::vector<uint32_t> table = deform_table(plan);

    // from here on the device: a HIP error drops the scene, since the description already holds the new arrays
    const DeformStage stage{staging, table, (uint32_t)plan.slots.size(), changed, deform_staging_capacity(mesh_n_vert.data(), mesh_n_tri.data(), mesh_n_tri.size()),
                            deform_table_slots_at(impl.instances.size()) + impl.meshes.size() * DEFORM_SLOT_WORDS};
    const SceneUpdateResult res = scene_update_step(&impl, SceneUpdate{rec, !rb.tris_are_local, plan.moved.data(), &light_pdf, true, rebuild_above, &stage});
    r.launches = res.launches; r.device_ms = res.device_ms;
    if (res.outcome == SceneUpdateResult::DEVICE_ERROR) return done(fail(MI355PT_E_DEVICE, res.what));
    if (res.outcome != SceneUpdateResult::DONE) return rebuild(res.outcome == SceneUpdateResult::SAH_DEGRADED ? MI355PT_MOVE_SAH_DEGRADED : MI355PT_MOVE_DEGENERATE_SET_CHANGED);
    r.sah_built = res.sah_built; r.sah_after = res.sah_after;
    r.reason = MI355PT_MOVE_REBASED;
    return done(MI355PT_OK);
}

int mi355pt_scene_debug_set_mesh_vertices(mi355pt_scene* s, const mi355pt_mesh_update* updates, uint32_t n) {
    if (!s || !updates || n == 0) return fail(MI355PT_E_INVALID, "null argument");
    if (s->impl.built || !s->parts.empty()) return fail(MI355PT_E_INVALID, "a built scene deforms with mi355pt_scene_deform_meshes");
    std::vector<Checked> ups;
    std::string err;
    if (!check_updates(s->impl, updates, n, &ups, &err)) return fail(MI355PT_E_INVALID, err);
    apply_updates(&s->impl, ups);
    return MI355PT_OK;
}

}  // extern "C"
