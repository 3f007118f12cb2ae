// Deforming meshes of a built scene (include/mi355pt_deform.h): the call itself and its host-only twin of the debug surface.  Host C++
// only; the kernel is pt_kernels_deform.hip, the rest of the move the instance move's launches (pt_kernels_rebase.hip,
// pt_kernels_instances.hip); the layout host and device share is deform_plan.hpp.  The side tables are RebaseState's (scene.hpp); the host
// form the tests hold the deformation to is mi355pt_scene_debug_pinned_digest (scene_rebase.cpp).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "api_internal.hpp"
#include "deform_plan.hpp"
#include "scene_lower.hpp"

using namespace pt;

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

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
    for (size_t k = 0; k + 1 < rb.left_out.size(); k += 2)        // a triangle the tree leaves out may no longer be degenerate (render space)
        if (plan.moved[rb.left_out[k]] && !render_triangle_degenerate(impl, rec.instances[rb.left_out[k]], rb.left_out[k], rb.left_out[k + 1])) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);
    if (rb.tris_are_local)                                        // ... and the local-space set, either way
        for (size_t k = 0; k < changed.size(); ++k) {
            const HostMesh& m = impl.meshes[changed[k].geom];
            for (uint32_t t = 0; t < m.n_tri; ++t) if ((local_triangle_degenerate(m, t) ? 1 : 0) != deg_before[k][t]) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);
        }

    DevScene& d = impl.dev;
    auto dropped = [&](const char* what, hipError_t e) { impl.release(); return done(fail(MI355PT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e))); };
    hipError_t e;
    hipStream_t stream = nullptr;
#if !PT_NODE_Q16
    const bool has_tree = d.root >= 0 && rb.n_entries > 0;
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
    const size_t n_inst = impl.instances.size();
    // the call's own buffers (the instance move's among them) and, once per build, the cost of the tree as it stands (nothing on the device
    // has changed yet, but the description already holds the new arrays, so a failure drops the scene all the same)
    if ((e = ensure(&impl, &rb.d_moved_bits, (n_inst + 31) / 32)) != hipSuccess || (e = ensure(&impl, &rb.d_light_pdf, light_pdf.size())) != hipSuccess ||
        (e = ensure(&impl, &rb.d_sah, sah_scratch_floats(rb.n_entries))) != hipSuccess ||
        (e = ensure(&impl, &rb.d_deform_staging, deform_staging_capacity(mesh_n_vert.data(), mesh_n_tri.data(), mesh_n_tri.size()))) != hipSuccess ||
        (e = ensure(&impl, &rb.d_deform_table, deform_table_slots_at(n_inst) + impl.meshes.size() * DEFORM_SLOT_WORDS)) != hipSuccess ||
        (e = ensure(&impl, &rb.d_mesh_idx, rb.mesh_idx_offset.back())) != hipSuccess) return dropped("hipMalloc", e);
    if (!rb.sah_built_valid) {
        rb.sah_built = 0.0f;
        if (has_tree) {
            if ((e = launch_sah_cost(d.nodes, d.root, rb.d_entries, rb.n_entries, rb.d_sah, stream)) != hipSuccess) return dropped("launch_sah_cost", e);
            if ((e = hipMemcpy(&rb.sah_built, rb.d_sah, sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return dropped("hipMemcpy", e);
        }
        rb.sah_built_valid = true;
    }
    std::vector<uint32_t> bits((n_inst + 31) / 32, 0u);
    for (size_t i = 0; i < plan.moved.size(); ++i) if (plan.moved[i]) bits[i >> 5] |= 1u << (i & 31u);
    for (const DeformUpdate& u : changed) {                       // a mesh's index buffer: once per build
        if (rb.mesh_idx_uploaded[u.geom]) continue;
        if ((e = hipMemcpy(rb.d_mesh_idx + rb.mesh_idx_offset[u.geom], impl.meshes[u.geom].idx.data(), (size_t)3 * u.n_tri * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
        rb.mesh_idx_uploaded[u.geom] = 1;
    }
    if ((e = hipMemcpy(rb.d_deform_staging, staging.data(), staging.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if ((e = hipMemcpy(rb.d_deform_table, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);

    // from here on the device records change: a HIP error leaves them half deformed, so the scene is dropped
    if ((e = hipMemcpy((void*)d.instances, rec.instances.data(), rec.instances.size() * sizeof(DevInstance), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!rec.lights.empty() && (e = hipMemcpy((void*)d.lights, rec.lights.data(), rec.lights.size() * sizeof(DevLight), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!rec.light_tris.empty() && (e = hipMemcpy((void*)d.light_tris, rec.light_tris.data(), rec.light_tris.size() * sizeof(DevLightTri), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if ((e = hipMemcpy(rb.d_moved_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!light_pdf.empty() && (e = hipMemcpy(rb.d_light_pdf, light_pdf.data(), light_pdf.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if ((e = hipMemset(rb.d_count, 0, sizeof(uint32_t))) != hipSuccess) return dropped("hipMemset", e);
    Event ev_a, ev_b;
    if ((e = ev_a.create()) != hipSuccess || (e = ev_b.create()) != hipSuccess) return dropped("hipEventCreate", e);
    if ((e = ev_a.record(stream)) != hipSuccess) return dropped("hipEventRecord", e);
    // tris_local is the array DevScene::tris names in local-triangle mode (scene.cpp upload): the traversals read what this launch writes,
    // and tris_render is re-derived from it by the next one in either mode
    if ((e = launch_deform_tris((DevTriLocal*)d.tris_local, (DevTriShade*)d.shade, rb.d_deform_table, rb.d_deform_staging, rb.d_mesh_idx, d.n_tris, (uint32_t)n_inst,
                                (uint32_t)deform_table_slots_at(n_inst), (uint32_t)plan.slots.size(), stream)) != hipSuccess) return dropped("launch_deform_tris", e);
    ++r.launches;
    if ((e = launch_rebase_tris(d.tris_local, d.instances, (DevTri*)d.tris_render, d.n_tris, !rb.tris_are_local, rb.d_count, stream)) != hipSuccess) return dropped("launch_rebase_tris", e);
    ++r.launches;
    if ((e = launch_shade_refresh((DevTriShade*)d.shade, d.tris_local, d.instances, rb.d_moved_bits, d.lights, rb.d_light_pdf, d.n_tris, (uint32_t)n_inst, d.n_lights,
                                  (uint32_t)light_pdf.size(), stream)) != hipSuccess) return dropped("launch_shade_refresh", e);
    ++r.launches;
    for (size_t h = 0; h + 1 < rb.height_offset.size(); ++h) {      // lowest height first: the kernel boundary orders the levels
        const uint32_t first = rb.height_offset[h], count = rb.height_offset[h + 1] - first;
        if (count == 0) continue;
        if ((e = launch_refit_bvh2_height((DevNode*)d.nodes, d.tris_render, rb.d_entries, first, count, stream)) != hipSuccess) return dropped("launch_refit_bvh2_height", e);
        ++r.launches;
    }
    if (rb.n_slots && d.root >= 0) {
        if ((e = launch_refit_nodes4((DevNode4*)d.nodes4, d.nodes, rb.d_slot_src, rb.n_slots, d.root, stream)) != hipSuccess) return dropped("launch_refit_nodes4", e);
        ++r.launches;
    }
    if (has_tree) {
        if ((e = launch_sah_cost(d.nodes, d.root, rb.d_entries, rb.n_entries, rb.d_sah, stream)) != hipSuccess) return dropped("launch_sah_cost", e);
        r.launches += SAH_COST_LAUNCHES;
    }
    if ((e = ev_b.record(stream)) != hipSuccess || (e = ev_b.synchronize()) != hipSuccess) return dropped("hipEventSynchronize", e);
    float ms = 0.0f;
    if ((e = ev_b.elapsed_ms(ev_a, &ms)) != hipSuccess) return dropped("hipEventElapsedTime", e);
    r.device_ms = ms;
    uint32_t n_degenerate = 0;
    if ((e = hipMemcpy(&n_degenerate, rb.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost)) != hipSuccess) return dropped("hipMemcpy", e);
    if (n_degenerate) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);      // (the build overwrites everything the launches wrote)
    float sah_after = 0.0f;
    if (has_tree && (e = hipMemcpy(&sah_after, rb.d_sah, sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return dropped("hipMemcpy", e);
    if (rebuild_above > 0.0f && rb.sah_built > 0.0f && sah_after / rb.sah_built > rebuild_above) return rebuild(MI355PT_MOVE_SAH_DEGRADED);
    r.sah_built = rb.sah_built; r.sah_after = sah_after;
#else
    return rebuild(MI355PT_MOVE_UNSUPPORTED_BUILD);
#endif
    // the caches the next move (of the camera, of instances, of vertices) starts from
    rb.lights = rec.lights;
    rb.light_tris = rec.light_tris;
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
