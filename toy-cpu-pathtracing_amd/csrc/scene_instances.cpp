// Moving instances of a built scene (include/mi355pt_instances.h): the dynamic mark and the move itself.  Host C++ only; the kernels are
// pt_kernels_rebase.hip (positions, both trees) and pt_kernels_instances.hip (shading records, SAH cost), the arithmetic both sides share
// instance_move_plan.hpp and rebase_plan.hpp.  The side tables are RebaseState's (scene.hpp, scene_rebase.cpp prepare_rebase); the host
// form the tests hold the move to is mi355pt_scene_debug_pinned_digest (scene_rebase.cpp).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "api_internal.hpp"
#include "instance_move_plan.hpp"
#include "scene_lower.hpp"

using namespace pt;

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

extern "C" {

int mi355pt_scene_set_instance_dynamic(mi355pt_scene* s, uint32_t instance, uint32_t dynamic) {
    if (!s) return fail(MI355PT_E_INVALID, "null argument");
    if (s->impl.built || !s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_set_instance_dynamic takes effect at a build: call it before mi355pt_scene_build");
    if (instance >= s->impl.instances.size()) return fail(MI355PT_E_INVALID, "bad instance id");
    s->impl.instances[instance].dynamic = dynamic ? 1u : 0u;
    return MI355PT_OK;
}

int mi355pt_scene_move_instances(mi355pt_scene* s, const mi355pt_camera* cam, const uint32_t* ids, const float* l2w, uint32_t n, const mi355pt_instance_move_params* p,
                                 mi355pt_instance_move_result* out) {
    const auto t0 = std::chrono::steady_clock::now();
    mi355pt_instance_move_result r{};
    if (out) *out = r;
    if (!s || !cam || !ids || !l2w || n == 0) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_move_instances does not move a scene built with mi355pt_scene_build_multi: build it again");
    SceneImpl& impl = s->impl;
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    for (uint32_t k = 0; k < n; ++k) {
        if (ids[k] >= impl.instances.size()) return fail(MI355PT_E_INVALID, "bad instance id");
        if (k && ids[k] <= ids[k - 1]) return fail(MI355PT_E_INVALID, "instance ids must be strictly ascending");
    }
    if (std::memcmp(cam->position, impl.build_cam_pos, sizeof(float) * 3) != 0) return fail(MI355PT_E_INVALID, "camera position differs from the position the scene is at: call mi355pt_scene_move_camera first");
    for (uint32_t k = 0; k < n; ++k)
        if (!instance_transform_ok(impl, cam, l2w + 16 * (size_t)k)) return fail(MI355PT_E_INVALID, "non-finite or singular instance transform");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    const float rebuild_above = p ? p->rebuild_above : 0.0f;
    if (p && !(rebuild_above >= 0.0f)) return fail(MI355PT_E_INVALID, "rebuild_above must be 0 or positive");
    auto done = [&](int rc) { r.host_ms = ms_since(t0); if (out) *out = r; return rc; };

    std::vector<uint8_t> moved(impl.instances.size(), 0);
    bool any = false;
    for (uint32_t k = 0; k < n; ++k)
        if (std::memcmp(impl.instances[ids[k]].l2w, l2w + 16 * (size_t)k, sizeof(float) * 16) != 0) { moved[ids[k]] = 1; any = true; }
    if (!any) { r.reason = MI355PT_MOVE_SAME_TRANSFORMS; return done(MI355PT_OK); }
    // the description takes the new matrices now: everything below — the records, the checks, a rebuild — is computed from it
    for (uint32_t k = 0; k < n; ++k) std::memcpy(impl.instances[ids[k]].l2w, l2w + 16 * (size_t)k, sizeof(float) * 16);
    auto rebuild = [&](uint32_t reason) { r.rebuilt = 1; r.reason = reason; r.launches = 0; r.device_ms = 0.0; r.sah_built = r.sah_after = 0.0f; return done(mi355pt_scene_build(s, cam)); };
    RebaseState& rb = impl.rebase;
    if (!rb.ready) return rebuild(MI355PT_MOVE_UNSUPPORTED_BUILD);

    // host: the small records with the lowering's own functions, the moved area lights' tables; then the cases in which a move in place is
    // not what a fresh lowering gives, in the camera move's order
    CameraRecords rec;
    std::vector<float> light_pdf;
    std::string err;
    if (int rc = lower_camera_records(impl, cam, rb.bounds, rb.lights, rb.light_tris, &rec, &err, moved.data(), &light_pdf)) return done(fail(rc, err));
    bool same_class = rec.tris_are_local == rb.tris_are_local && !rb.tris_are_local && rec.instances.size() == rb.identity.size();   // (local-triangle mode: every instance shares ONE translation)
    for (size_t i = 0; same_class && i < rec.instances.size(); ++i) same_class = (rec.instances[i].identity != 0) == (rb.identity[i] != 0);
    if (!same_class) return rebuild(MI355PT_MOVE_INSTANCE_CLASS_CHANGED);
    for (size_t k = 0; k + 1 < rb.left_out.size(); k += 2)        // a triangle the tree leaves out may no longer be degenerate
        if (moved[rb.left_out[k]] && !render_triangle_degenerate(impl, rec.instances[rb.left_out[k]], rb.left_out[k], rb.left_out[k + 1])) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);

    DevScene& d = impl.dev;
    auto dropped = [&](const char* what, hipError_t e) { impl.release(); return done(fail(MI355PT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e))); };
    hipError_t e;
    hipStream_t stream = nullptr;
#if !PT_NODE_Q16
    const bool has_tree = d.root >= 0 && rb.n_entries > 0;
    // the move's own buffers and, once per build, the cost of the tree as it stands (nothing of the scene has changed yet: a failure here
    // leaves it as it was, but the description already holds the new matrices, so the scene is dropped all the same)
    if ((e = ensure(&impl, &rb.d_moved_bits, (impl.instances.size() + 31) / 32)) != hipSuccess || (e = ensure(&impl, &rb.d_light_pdf, light_pdf.size())) != hipSuccess ||
        (e = ensure(&impl, &rb.d_sah, sah_scratch_floats(rb.n_entries))) != hipSuccess) return dropped("hipMalloc", e);
    if (!rb.sah_built_valid) {
        rb.sah_built = 0.0f;
        if (has_tree) {
            if ((e = launch_sah_cost(d.nodes, d.root, rb.d_entries, rb.n_entries, rb.d_sah, stream)) != hipSuccess) return dropped("launch_sah_cost", e);
            if ((e = hipMemcpy(&rb.sah_built, rb.d_sah, sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return dropped("hipMemcpy", e);
        }
        rb.sah_built_valid = true;
    }
    std::vector<uint32_t> bits((impl.instances.size() + 31) / 32, 0u);
    for (size_t i = 0; i < moved.size(); ++i) if (moved[i]) bits[i >> 5] |= 1u << (i & 31u);

    // from here on the device records change: a HIP error leaves them half moved, so the scene is dropped
    if ((e = hipMemcpy((void*)d.instances, rec.instances.data(), rec.instances.size() * sizeof(DevInstance), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!rec.lights.empty() && (e = hipMemcpy((void*)d.lights, rec.lights.data(), rec.lights.size() * sizeof(DevLight), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!rec.light_tris.empty() && (e = hipMemcpy((void*)d.light_tris, rec.light_tris.data(), rec.light_tris.size() * sizeof(DevLightTri), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if ((e = hipMemcpy(rb.d_moved_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if (!light_pdf.empty() && (e = hipMemcpy(rb.d_light_pdf, light_pdf.data(), light_pdf.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return dropped("hipMemcpy", e);
    if ((e = hipMemset(rb.d_count, 0, sizeof(uint32_t))) != hipSuccess) return dropped("hipMemset", e);
    Event ev_a, ev_b;
    if ((e = ev_a.create()) != hipSuccess || (e = ev_b.create()) != hipSuccess) return dropped("hipEventCreate", e);
    if ((e = ev_a.record(stream)) != hipSuccess) return dropped("hipEventRecord", e);
    if ((e = launch_rebase_tris(d.tris_local, d.instances, (DevTri*)d.tris_render, d.n_tris, true, rb.d_count, stream)) != hipSuccess) return dropped("launch_rebase_tris", e);
    ++r.launches;
    if ((e = launch_shade_refresh((DevTriShade*)d.shade, d.tris_local, d.instances, rb.d_moved_bits, d.lights, rb.d_light_pdf, d.n_tris, (uint32_t)impl.instances.size(),
                                  d.n_lights, (uint32_t)light_pdf.size(), stream)) != hipSuccess) return dropped("launch_shade_refresh", e);
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
    // the caches the next move (of the camera or of instances) starts from
    rb.lights = rec.lights;
    rb.light_tris = rec.light_tris;
    r.reason = MI355PT_MOVE_REBASED;
    return done(MI355PT_OK);
}

}  // extern "C"
