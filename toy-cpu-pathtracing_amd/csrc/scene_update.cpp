// The device step of an in-place update of a built scene (scene_update.hpp): uploads, launches and read-backs in their one order.
// Host C++ only; the kernels are pt_kernels_rebase.hip (positions, both trees), pt_kernels_instances.hip (shading records, SAH cost), pt_kernels_deform.hip.
#include "scene_update.hpp"

#include "path_end_plan.hpp"

namespace pt {

SceneUpdateResult scene_update_step(SceneImpl* impl, const SceneUpdate& u) {
    SceneUpdateResult r;
    // the description already holds the new values and, past the first upload, the device records are half updated: a HIP error drops the scene
    auto dropped = [&](const char* what, hipError_t e) { impl->release(); r.outcome = SceneUpdateResult::DEVICE_ERROR; r.what = std::string(what) + ": " + hipGetErrorString(e); return r; };
#define STEP_TRY(what, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return dropped(what, _e); } while (0)
#if PT_NODE_Q16
    return dropped("scene_update_step", hipErrorNotSupported);     // (not reached: such a build is never rebase.ready)
#else
    RebaseState& rb = impl->rebase;
    DevScene& d = impl->dev;
    hipStream_t stream = nullptr;
    if (u.edit) {
        // an edit of materials and lights: uploads into the build's allocations, each of the array's built size, and at most one launch
        const EditStage& e = *u.edit;
        size_t n_cc = 0;
        for (const DevMaterial& m : rb.materials) if (m.type == MT_CLEARCOAT) ++n_cc;
        if ((e.materials && e.materials->size() != (size_t)d.n_materials) || (e.cc_albedo && e.cc_albedo->size() != std::max<size_t>(n_cc, 1) * 64) ||
            (e.lights && e.lights->size() != (size_t)d.n_lights) || (e.envs && (e.envs->size() != (size_t)d.n_envs || !e.env_tables || !e.env_map_changed)) ||
            (e.class_table && (e.class_table->size() != (size_t)d.n_materials || !rb.d_class_table)))
            return dropped("scene_update_step: a record list changed size since the build", hipErrorInvalidValue);
        if (e.envs) {
            std::vector<DevEnv> envs(d.n_envs);                                // the built records name the tables on the device
            if (d.n_envs) STEP_TRY("hipMemcpy", hipMemcpy(envs.data(), d.envs, envs.size() * sizeof(DevEnv), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < envs.size(); ++k) {
                const DevEnv& built = envs[k];
                DevEnv ne = (*e.envs)[k];
                if (ne.w != built.w || ne.h != built.h) return dropped("scene_update_step: an environment map changed size since the build", hipErrorInvalidValue);
                ne.texels = built.texels; ne.marginal = built.marginal; ne.conditional = built.conditional;
                if (e.env_map_changed[k]) {
                    const LoweredScene::EnvTables& t = (*e.env_tables)[k];
                    const size_t px = (size_t)ne.w * ne.h;
                    if (t.texels.size() != px * 4 || t.marginal.size() != (size_t)ne.h || t.conditional.size() != px) return dropped("scene_update_step: environment tables of another size", hipErrorInvalidValue);
                    STEP_TRY("hipMemcpy", hipMemcpy((void*)ne.texels, t.texels.data(), t.texels.size() * sizeof(float), hipMemcpyHostToDevice));
                    STEP_TRY("hipMemcpy", hipMemcpy((void*)ne.marginal, t.marginal.data(), t.marginal.size() * sizeof(float), hipMemcpyHostToDevice));
                    STEP_TRY("hipMemcpy", hipMemcpy((void*)ne.conditional, t.conditional.data(), t.conditional.size() * sizeof(float), hipMemcpyHostToDevice));
                }
                envs[k] = ne;
            }
            if (d.n_envs) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.envs, envs.data(), envs.size() * sizeof(DevEnv), hipMemcpyHostToDevice));
        }
        if (e.cc_albedo) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.cc_albedo, e.cc_albedo->data(), e.cc_albedo->size() * sizeof(float), hipMemcpyHostToDevice));
        if (e.materials) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.materials, e.materials->data(), e.materials->size() * sizeof(DevMaterial), hipMemcpyHostToDevice));
        // (the lights' boxes behind the records are the emissive triangles': no edit moves them)
        if (e.lights) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.lights, e.lights->data(), e.lights->size() * sizeof(DevLight), hipMemcpyHostToDevice));
        if (e.class_table) {
            STEP_TRY("hipMemcpy", hipMemcpy(rb.d_class_table, e.class_table->data(), e.class_table->size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            Event ev_a, ev_b;
            STEP_TRY("hipEventCreate", ev_a.create()); STEP_TRY("hipEventCreate", ev_b.create());
            STEP_TRY("hipEventRecord", ev_a.record(stream));
            // DevScene::tris is one of the two arrays (scene.cpp upload); were it a third, it would carry the class too
            DevTri* walked = d.tris != d.tris_local && d.tris != d.tris_render ? (DevTri*)d.tris : nullptr;
            STEP_TRY("launch_reclass_tris", launch_reclass_tris((DevTriLocal*)d.tris_local, (DevTri*)d.tris_render, walked, d.shade, rb.d_class_table, d.n_tris, d.n_materials, stream));
            ++r.launches;
            STEP_TRY("hipEventRecord", ev_b.record(stream)); STEP_TRY("hipEventSynchronize", ev_b.synchronize());
            float ms = 0.0f;
            STEP_TRY("hipEventElapsedTime", ev_b.elapsed_ms(ev_a, &ms)); r.device_ms = ms;
        }
        return r;
    }
    const size_t n_inst = impl->instances.size(), n_pdf = u.light_pdf ? u.light_pdf->size() : 0;
    const bool has_tree = u.sah && d.root >= 0 && rb.n_entries > 0;

    // the update's own buffers, allocated by the first call after a build that needs them, and, once per build, the cost of the tree as it stands
    if (u.moved) { STEP_TRY("hipMalloc", ensure(impl, &rb.d_moved_bits, (n_inst + 31) / 32)); STEP_TRY("hipMalloc", ensure(impl, &rb.d_light_pdf, n_pdf)); }
    if (u.sah) STEP_TRY("hipMalloc", ensure(impl, &rb.d_sah, sah_scratch_floats(rb.n_entries)));
    if (u.deform) { STEP_TRY("hipMalloc", ensure(impl, &rb.d_deform_staging, u.deform->staging_capacity)); STEP_TRY("hipMalloc", ensure(impl, &rb.d_deform_table, u.deform->table_capacity)); }
    if (u.deform) STEP_TRY("hipMalloc", ensure(impl, &rb.d_mesh_idx, rb.mesh_idx_offset.back()));
    if (u.sah && !rb.sah_built_valid) {
        rb.sah_built = 0.0f;
        if (has_tree) {
            STEP_TRY("launch_sah_cost", launch_sah_cost(d.nodes, d.root, rb.d_entries, rb.n_entries, rb.d_sah, stream));
            STEP_TRY("hipMemcpy", hipMemcpy(&rb.sah_built, rb.d_sah, sizeof(float), hipMemcpyDeviceToHost));
        }
        rb.sah_built_valid = true;
    }
    if (u.deform) {
        for (const DeformUpdate& m : u.deform->meshes) {               // a mesh's index buffer: once per build
            if (rb.mesh_idx_uploaded[m.geom]) continue;
            STEP_TRY("hipMemcpy", hipMemcpy(rb.d_mesh_idx + rb.mesh_idx_offset[m.geom], impl->meshes[m.geom].idx.data(), (size_t)3 * m.n_tri * sizeof(uint32_t), hipMemcpyHostToDevice));
            rb.mesh_idx_uploaded[m.geom] = 1;
        }
        STEP_TRY("hipMemcpy", hipMemcpy(rb.d_deform_staging, u.deform->staging.data(), u.deform->staging.size() * sizeof(float), hipMemcpyHostToDevice));
        STEP_TRY("hipMemcpy", hipMemcpy(rb.d_deform_table, u.deform->table.data(), u.deform->table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }

    // (the light allocation is n_lights records and n_lights boxes, path_end_plan.hpp light_allocation_bytes: the copies below rely on the count)
    if (!u.rec.lights.empty() && u.rec.lights.size() != (size_t)d.n_lights) return dropped("scene_update_step: light list changed since the build", hipErrorInvalidValue);
    // from here on the device records change
    STEP_TRY("hipMemcpy", hipMemcpy((void*)d.instances, u.rec.instances.data(), u.rec.instances.size() * sizeof(DevInstance), hipMemcpyHostToDevice));
    if (!u.rec.lights.empty()) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.lights, u.rec.lights.data(), u.rec.lights.size() * sizeof(DevLight), hipMemcpyHostToDevice));
    if (!u.rec.light_tris.empty()) STEP_TRY("hipMemcpy", hipMemcpy((void*)d.light_tris, u.rec.light_tris.data(), u.rec.light_tris.size() * sizeof(DevLightTri), hipMemcpyHostToDevice));
    if (!u.rec.lights.empty()) {
        // the lights' boxes, behind the light records (scene.cpp upload): from the triangles written above, in the same step
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        std::vector<float> boxes;
        light_boxes(u.rec.lights, u.rec.light_tris, u.rec.tris_are_local ? u.rec.shared_iw : zero, &boxes);
        STEP_TRY("hipMemcpy", hipMemcpy((void*)light_box_of(d.lights, d.n_lights, 0u), boxes.data(), boxes.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (u.moved) {
        std::vector<uint32_t> bits((n_inst + 31) / 32, 0u);
        for (size_t i = 0; i < n_inst; ++i) if (u.moved[i]) bits[i >> 5] |= 1u << (i & 31u);
        STEP_TRY("hipMemcpy", hipMemcpy(rb.d_moved_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (n_pdf) STEP_TRY("hipMemcpy", hipMemcpy(rb.d_light_pdf, u.light_pdf->data(), n_pdf * sizeof(float), hipMemcpyHostToDevice));
    }
    STEP_TRY("hipMemset", hipMemset(rb.d_count, 0, sizeof(uint32_t)));
    Event ev_a, ev_b;
    STEP_TRY("hipEventCreate", ev_a.create()); STEP_TRY("hipEventCreate", ev_b.create());
    STEP_TRY("hipEventRecord", ev_a.record(stream));
    if (u.deform) {
        // tris_local is the array DevScene::tris names in local-triangle mode (scene.cpp upload): the traversals read what this launch writes,
        // and tris_render is re-derived from it by the next one in either mode
        STEP_TRY("launch_deform_tris", launch_deform_tris((DevTriLocal*)d.tris_local, (DevTriShade*)d.shade, rb.d_deform_table, rb.d_deform_staging, rb.d_mesh_idx, d.n_tris,
                                                          (uint32_t)n_inst, (uint32_t)deform_table_slots_at(n_inst), u.deform->n_slots, stream));
        ++r.launches;
    }
    STEP_TRY("launch_rebase_tris", launch_rebase_tris(d.tris_local, d.instances, (DevTri*)d.tris_render, d.n_tris, u.count_degenerate, rb.d_count, stream));
    ++r.launches;
    if (u.moved) {
        STEP_TRY("launch_shade_refresh", launch_shade_refresh((DevTriShade*)d.shade, d.tris_local, d.instances, rb.d_moved_bits, d.lights, rb.d_light_pdf, d.n_tris, (uint32_t)n_inst,
                                                              d.n_lights, (uint32_t)n_pdf, stream));
        ++r.launches;
    }
    for (size_t h = 0; h + 1 < rb.height_offset.size(); ++h) {      // lowest height first: the kernel boundary orders the levels
        const uint32_t first = rb.height_offset[h], count = rb.height_offset[h + 1] - first;
        if (count == 0) continue;
        STEP_TRY("launch_refit_bvh2_height", launch_refit_bvh2_height((DevNode*)d.nodes, d.tris_render, rb.d_entries, first, count, stream));
        ++r.launches;
    }
    if (rb.n_slots && d.root >= 0) {
        STEP_TRY("launch_refit_nodes4", launch_refit_nodes4((DevNode4*)d.nodes4, d.nodes, rb.d_slot_src, rb.n_slots, d.root, stream));
        ++r.launches;
    }
    if (has_tree) {
        STEP_TRY("launch_sah_cost", launch_sah_cost(d.nodes, d.root, rb.d_entries, rb.n_entries, rb.d_sah, stream));
        r.launches += SAH_COST_LAUNCHES;
    }
    STEP_TRY("hipEventSynchronize", ev_b.record(stream)); STEP_TRY("hipEventSynchronize", ev_b.synchronize());
    float ms = 0.0f;
    STEP_TRY("hipEventElapsedTime", ev_b.elapsed_ms(ev_a, &ms)); r.device_ms = ms;
    uint32_t n_degenerate = 0;
    STEP_TRY("hipMemcpy", hipMemcpy(&n_degenerate, rb.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_degenerate) { r.outcome = SceneUpdateResult::DEGENERATE_SET_CHANGED; return r; }
    if (u.sah) {
        if (has_tree) STEP_TRY("hipMemcpy", hipMemcpy(&r.sah_after, rb.d_sah, sizeof(float), hipMemcpyDeviceToHost));
        r.sah_built = rb.sah_built;
        if (u.rebuild_above > 0.0f && rb.sah_built > 0.0f && r.sah_after / rb.sah_built > u.rebuild_above) { r.outcome = SceneUpdateResult::SAH_DEGRADED; return r; }
    }
    // the caches the next update starts from: what the device holds now (a camera move re-lowers the delta lights' render-space positions
    // too, and mi355pt_scene_edit compares its records with these)
    if (!u.rec.lights.empty()) rb.lights = u.rec.lights;
    if (!u.rec.light_tris.empty()) rb.light_tris = u.rec.light_tris;
    return r;
#endif
#undef STEP_TRY
}

}  // namespace pt
