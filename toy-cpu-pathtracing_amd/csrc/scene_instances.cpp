// Moving instances of a built scene (include/mi355pt_instances.h): the dynamic mark and the move itself.  Host C++ only; the device half
// is scene_update.cpp's step, the kernels are pt_kernels_rebase.hip (positions, both trees) and pt_kernels_instances.hip (shading records,
// SAH cost), the arithmetic both sides share instance_move_plan.hpp and rebase_plan.hpp.  The side tables are RebaseState's (scene.hpp,
// scene_rebase.cpp prepare_rebase); the host form the tests hold the move to is mi355pt_scene_debug_pinned_digest (scene_debug.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "scene_update.hpp"

using namespace pt;

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
    if (rb.tris_are_local || !same_lowering_class(rec.instances, rec.tris_are_local, rb.identity, rb.tris_are_local)) return rebuild(MI355PT_MOVE_INSTANCE_CLASS_CHANGED);   // (local-triangle mode: every instance shares ONE translation)
    if (!left_out_stay_degenerate(impl, rec.instances, moved.data())) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);   // a triangle the tree leaves out may no longer be degenerate

    // from here on the device: a HIP error drops the scene, since the description already holds the new matrices
    const SceneUpdateResult res = scene_update_step(&impl, SceneUpdate{rec, true, moved.data(), &light_pdf, true, rebuild_above});
    r.launches = res.launches; r.device_ms = res.device_ms;
    if (res.outcome == SceneUpdateResult::DEVICE_ERROR) return done(fail(MI355PT_E_DEVICE, res.what));
    if (res.outcome != SceneUpdateResult::DONE) return rebuild(res.outcome == SceneUpdateResult::SAH_DEGRADED ? MI355PT_MOVE_SAH_DEGRADED : MI355PT_MOVE_DEGENERATE_SET_CHANGED);
    r.sah_built = res.sah_built; r.sah_after = res.sah_after;
    r.reason = MI355PT_MOVE_REBASED;
    return done(MI355PT_OK);
}

}  // extern "C"
