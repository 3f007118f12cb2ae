// The mi355pt_flow.h surface of libmi355pt.so: the mark (a scene-owned copy of last frame's triangle positions), the flow pass (the ID
// pass's launch, api_motion.cpp, with a motion record per pixel) and the four flow forms of the temporal accumulation: single calls of
// api_temporal.cpp's driver with a flow carry, whose own check (flow_checks.hpp) is here.  Host C++ only, like api.cpp; the flow pass's
// kernels are in pt_kernels_flow.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "api_internal.hpp"
#include "flow_checks.hpp"

using namespace pt;

static_assert(sizeof(mi355pt_flow_pixel) == sizeof(FlowPixelDev) && sizeof(mi355pt_flow_pixel) == 32, "one layout of a flow record");

// every check of the flow pass's entry points; host memory only.  The pointer checks come first: they need no scene
int pt::flow_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const void* flow, size_t flow_align, const void* ids) {
    switch (flow_out_verdict(flow, flow_align, ids)) {
        case FlowOut::MISSING: return fail(MI355PT_E_INVALID, "flow: null record buffer");
        case FlowOut::MISALIGNED: return fail(MI355PT_E_INVALID, "flow: the record buffer must be 16-byte aligned");
        case FlowOut::SAME_BUFFER: return fail(MI355PT_E_INVALID, "flow: the record buffer must not be the id buffer");
        case FlowOut::OK: break;
    }
    const int rc = ids_check(s, cam, p, flow);
    if (rc) return rc;
    if (!s->impl.rebase.flow_marked) return fail(MI355PT_E_INVALID, "flow: the scene holds no mark (mi355pt_scene_flow_mark; every build drops it)");
    if (s->impl.dev.n_tris == 0u) return fail(MI355PT_E_INVALID, "flow: the scene has no triangles");
    return MI355PT_OK;
}

// the launch of mi355pt_render_flow_device, arguments checked (mi355pt_render_ids_device's, with the flow kernel)
int pt::render_flow_launch(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, mi355pt_flow_pixel* d_flow, uint32_t* d_ids, void* d_hits,
                           void* hip_stream, mi355pt_stats* stats) {
    if (shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) == 0) return MI355PT_OK;
    LaunchCtx* lc; int slot, rc;
    if ((rc = get_launch_ctx(s, p->seed, &lc, &slot))) return rc;
    if (lc->device != s->impl.device) return fail(MI355PT_E_DEVICE, "launch context and scene live on different devices");
    int& waves = lc->flow_waves[d_hits ? 1 : 0];
    if (!waves) waves = query_resident_waves_flow(d_hits != nullptr);
    const DevCamera dc = make_camera(cam);
    LaunchPlan plan = plan_ids(cam, p, waves);
    plan.params.stats_mode = 0u;
    const hipStream_t stream = (hipStream_t)hip_stream;
    return timed_launch(lc, slot, stream, stats, true, [&](unsigned* d_counter, DevStats* d_stats) {
        HIP_TRY(launch_flow(s->impl.dev, dc, plan.params, s->impl.rebase.d_tris_prev, (FlowPixelDev*)d_flow, d_ids, d_hits, d_counter, stats ? d_stats : nullptr,
                            plan.grid, stream));
        return (int)MI355PT_OK;
    });
}

// what mi355pt_flow.h adds to temporal_check (and, with a scratch, to the rectified form's checks)
int pt::flow_in_check(const TemporalCarry& carry, const TemporalCall& c, const void* scratch) {
    const void* outs[4] = {c.out_film, c.out_half, c.out_length, scratch};
    switch (flow_in_verdict(carry.ids_cur, carry.ids_prev, carry.flow, carry.align, outs, 4)) {
        case FlowIn::MISSING: return fail(MI355PT_E_INVALID, "temporal flow: null record buffer");
        case FlowIn::MISALIGNED: return fail(MI355PT_E_INVALID, "temporal flow: the record buffer must be 16-byte aligned");
        case FlowIn::PREV_IDS_ALONE: return fail(MI355PT_E_INVALID, "temporal flow: the previous frame's ids need the current frame's");
        case FlowIn::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "temporal flow: the records or an id buffer must not be an output or the scratch");
        case FlowIn::OK: break;
    }
    return MI355PT_OK;
}

namespace {

TemporalCarry flow_carry(const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_flow_pixel* flow, size_t align) {
    TemporalCarry carry;
    carry.kind = TemporalCarry::FLOW; carry.ids_cur = ids_cur; carry.ids_prev = ids_prev; carry.flow = flow; carry.align = align;
    return carry;
}

}  // namespace

extern "C" {

int mi355pt_scene_flow_mark(mi355pt_scene* s, void* hip_stream) {
    if (!s) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_flow_mark does not mark a scene built with mi355pt_scene_build_multi");
    SceneImpl& impl = s->impl;
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    RebaseState& rb = impl.rebase;
    const size_t n = impl.dev.n_tris;
    HIP_TRY(ensure(&impl, &rb.d_tris_prev, n));
    if (n) HIP_TRY(hipMemcpyAsync(rb.d_tris_prev, impl.dev.tris_render, n * sizeof(DevTri), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    rb.flow_marked = true;
    return MI355PT_OK;
}

int mi355pt_scene_flow_marked(const mi355pt_scene* s) { return s && s->impl.built && s->impl.rebase.flow_marked ? 1 : 0; }

int mi355pt_render_flow_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, mi355pt_flow_pixel* d_flow, uint32_t* d_ids,
                               void* hip_stream, mi355pt_stats* stats) {
    const int rc = flow_check(s, cam, p, d_flow, 16, d_ids);
    if (rc) return rc;
    return render_flow_launch(s, cam, p, d_flow, d_ids, nullptr, hip_stream, stats);
}

int mi355pt_render_flow(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, mi355pt_flow_pixel* flow, uint32_t* ids, mi355pt_stats* stats) {
    int rc = flow_check(s, cam, p, flow, 1, ids);
    if (rc) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    DevBuf<mi355pt_flow_pixel> d_flow;
    DevBuf<uint32_t> d_ids;
    HIP_TRY(d_flow.alloc(np));
    HIP_TRY(hipMemset(d_flow.p, 0, np * sizeof(mi355pt_flow_pixel)));
    HIP_TRY(d_ids.alloc_for(ids, np));
    if (ids) HIP_TRY(hipMemset(d_ids.p, 0, np * sizeof(uint32_t)));
    if ((rc = render_flow_launch(s, cam, p, d_flow.p, d_ids.p, nullptr, nullptr, stats))) return rc;
    HIP_TRY(d_flow.download(flow, np));
    HIP_TRY(d_ids.download(ids, np));
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_flow_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                            uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* d_ids_cur,
                                            const uint32_t* d_ids_prev, const mi355pt_flow_pixel* d_flow, float* d_out_film, float* d_out_half,
                                            float* d_out_length, void* hip_stream) {
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length}, flow_carry(d_ids_cur, d_ids_prev, d_flow, 16),
                                      nullptr, hip_stream);
}

int mi355pt_temporal_accumulate_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                     uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                     const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length) {
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, flow_carry(ids_cur, ids_prev, flow, 1), nullptr);
}

int mi355pt_temporal_accumulate_rectified_flow_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                      const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                      const mi355pt_temporal_rectify_params* rp, void* d_scratch, size_t scratch_bytes, const uint32_t* d_ids_cur,
                                                      const uint32_t* d_ids_prev, const mi355pt_flow_pixel* d_flow, float* d_out_film, float* d_out_half,
                                                      float* d_out_length, void* hip_stream) {
    const TemporalRectify rect{rp, d_scratch, scratch_bytes};
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length}, flow_carry(d_ids_cur, d_ids_prev, d_flow, 16),
                                      &rect, hip_stream);
}

int mi355pt_temporal_accumulate_rectified_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                               const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                               const mi355pt_temporal_rectify_params* rp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                               const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length) {
    const TemporalRectify rect{rp};
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, flow_carry(ids_cur, ids_prev, flow, 1), &rect);
}

}  // extern "C"
