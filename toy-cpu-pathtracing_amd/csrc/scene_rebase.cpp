// Moving the camera of a built scene (include/mi355pt_rebase.h): the side tables SceneImpl::build leaves for it and for the two other
// updates in place, and the move itself.  Host C++ only; the device half is scene_update.cpp's step, the kernels are
// pt_kernels_rebase.hip, the plan and the arithmetic both sides share rebase_plan.hpp.  The digests the tests hold it to are scene_debug.cpp's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "rebase_plan.hpp"
#include "scene_update.hpp"

using namespace pt;

namespace {

int upload_words(SceneImpl* s, const std::vector<uint32_t>& v, uint32_t** out, std::string* err) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(v.size() * sizeof(uint32_t), 16));
    if (e != hipSuccess) { *err = std::string("hipMalloc: ") + hipGetErrorString(e); return MI355PT_E_DEVICE; }
    s->allocs.push_back(p);
    if (!v.empty() && (e = hipMemcpy(p, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) { *err = std::string("hipMemcpy: ") + hipGetErrorString(e); return MI355PT_E_DEVICE; }
    *out = (uint32_t*)p;
    return MI355PT_OK;
}

}  // namespace

int SceneImpl::prepare_rebase(const LoweredScene& ls, const LowerReport& rep, std::string* err, bool on_device) {
    RebaseState& rb = rebase;
    rb.ready = false; rb.pinned = false;
    rb.n_degenerate = rep.n_degenerate; rb.bvh_depth = rep.bvh_depth; rb.stack_need = rep.stack_need; rb.collapse_method = rep.collapse_method;
#if !PT_NODE_Q16
    RebasePlan plan;
    if (!make_rebase_plan(ls.nodes, ls.dev.root, ls.nodes4, ls.dev.root4, ls.tris_render.size(), &plan)) return MI355PT_OK;   // (a tree the plan does not cover: a move builds again)
    int rc;
    if (on_device && ((rc = upload_words(this, plan.entries, &rb.d_entries, err)) || (rc = upload_words(this, plan.slot_src, &rb.d_slot_src, err)) ||
                      (rc = upload_words(this, std::vector<uint32_t>(4, 0u), &rb.d_count, err)) ||
                      (rc = upload_words(this, std::vector<uint32_t>(ls.materials.size(), 0xffffffffu), &rb.d_class_table, err)))) return rc;
    rb.height_offset = plan.height_offset;
    rb.n_slots = (uint32_t)plan.slot_src.size();
    rb.n_entries = (uint32_t)plan.entries.size();
    rb.tree_nodes4 = ls.nodes4; rb.tree_root4 = ls.dev.root4;
    rb.identity.resize(ls.instances.size());
    for (size_t i = 0; i < ls.instances.size(); ++i) rb.identity[i] = (uint8_t)ls.instances[i].identity;
    rb.tris_are_local = ls.dev.tris_are_local != 0;
    mesh_local_bounds(*this, &rb.bounds);
    rb.lights = ls.lights;
    rb.light_tris = ls.light_tris;
    rb.materials = ls.materials; rb.cc_albedo = ls.cc_albedo; rb.textures = ls.textures; rb.n_luts = (uint32_t)luts.size(); rb.envs = ls.envs;
    rb.pinned = true;
    rb.ready = on_device;
#endif
    return MI355PT_OK;
}

extern "C" {

int mi355pt_scene_move_camera(mi355pt_scene* s, const mi355pt_camera* cam, mi355pt_move_result* out) {
    const auto t0 = std::chrono::steady_clock::now();
    mi355pt_move_result r{};
    if (out) *out = r;
    if (!s || !cam) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_move_camera does not move a scene built with mi355pt_scene_build_multi: build it again");
    SceneImpl& impl = s->impl;
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    auto done = [&](int rc) { r.host_ms = ms_since(t0); if (out) *out = r; return rc; };
    if (std::memcmp(cam->position, impl.build_cam_pos, sizeof(float) * 3) == 0) { r.reason = MI355PT_MOVE_SAME_POSITION; return done(MI355PT_OK); }
    auto rebuild = [&](uint32_t reason) { r.rebuilt = 1; r.reason = reason; r.launches = 0; r.device_ms = 0.0; return done(mi355pt_scene_build(s, cam)); };
    const RebaseState& rb = impl.rebase;
    if (!rb.ready) return rebuild(MI355PT_MOVE_UNSUPPORTED_BUILD);

    // host: the small records, with the lowering's own functions; then the two cases in which re-basing is not what a fresh lowering gives
    CameraRecords rec;
    std::string err;
    if (int rc = lower_camera_records(impl, cam, rb.bounds, rb.lights, rb.light_tris, &rec, &err)) return done(fail(rc, err));
    if (!same_lowering_class(rec.instances, rec.tris_are_local, rb.identity, rb.tris_are_local)) return rebuild(MI355PT_MOVE_INSTANCE_CLASS_CHANGED);
    if (!left_out_stay_degenerate(impl, rec.instances)) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);   // a triangle the tree leaves out may no longer be degenerate

    // from here on the device records change: a HIP error leaves them half moved, so the scene is dropped
    const SceneUpdateResult res = scene_update_step(&impl, SceneUpdate{rec, !rb.tris_are_local});
    r.launches = res.launches; r.device_ms = res.device_ms;
    if (res.outcome == SceneUpdateResult::DEVICE_ERROR) return done(fail(MI355PT_E_DEVICE, res.what));
    if (res.outcome != SceneUpdateResult::DONE) return rebuild(MI355PT_MOVE_DEGENERATE_SET_CHANGED);      // (the build overwrites everything the launches wrote)

    DevScene& d = impl.dev;
    for (int k = 0; k < 3; ++k) { d.tri_shift[k] = rec.tris_are_local ? rec.shared_iw[k] : 0.0f; d.shared_mw[k] = rec.tris_are_local ? rec.shared_mw[k] : 0.0f; }
    std::memcpy(impl.build_cam_pos, cam->position, sizeof(impl.build_cam_pos));
    r.reason = MI355PT_MOVE_REBASED;
    return done(MI355PT_OK);
}

}  // extern "C"
