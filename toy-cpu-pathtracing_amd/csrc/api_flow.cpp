// The mi355pt_flow.h surface of libmi355pt.so: the mark (a scene-owned copy of last frame's triangle positions), the flow pass (the ID
// pass's launch, api_motion.cpp, with a motion record per pixel) and the flow-aware twins of the temporal accumulation and of its rectified
// form, which run api_temporal.cpp's checks and add their own (flow_checks.hpp).  Host C++ only, like api.cpp; the kernels are in
// pt_kernels_flow.hip and pt_kernels_temporal_flow.hip.
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

namespace {

// what mi355pt_flow.h adds to temporal_check (and, with a scratch, to the rectified form's checks)
int flow_in_check(const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_flow_pixel* flow, size_t flow_align, const void* out_film, const void* out_half,
                  const void* out_length, const void* scratch) {
    const void* outs[4] = {out_film, out_half, out_length, scratch};
    switch (flow_in_verdict(ids_cur, ids_prev, flow, flow_align, outs, 4)) {
        case FlowIn::MISSING: return fail(MI355PT_E_INVALID, "temporal flow: null record buffer");
        case FlowIn::MISALIGNED: return fail(MI355PT_E_INVALID, "temporal flow: the record buffer must be 16-byte aligned");
        case FlowIn::PREV_IDS_ALONE: return fail(MI355PT_E_INVALID, "temporal flow: the previous frame's ids need the current frame's");
        case FlowIn::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "temporal flow: the records or an id buffer must not be an output or the scratch");
        case FlowIn::OK: break;
    }
    return MI355PT_OK;
}

// the two host-buffer entry points, after api_motion.cpp's motion_accumulate_host: device copies of the films, the ids and the records, the
// device entry point (rectified when rp is given, with a scratch of its own) on the default stream, the outputs copied back.  Every
// argument has been checked.
int flow_accumulate_host(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                         uint32_t height, const mi355pt_temporal_params* tp, const mi355pt_temporal_rectify_params* rp, const uint32_t* ids_cur,
                         const uint32_t* ids_prev, const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length) {
    int rc = MI355PT_OK;
    const size_t np = (size_t)width * height, n = np * 3;
    DevBuf<float> d_in[2][6], d_film, d_half, d_len;
    DevBuf<uint32_t> d_ids[2];
    DevBuf<mi355pt_flow_pixel> d_flow;
    DevBuf<unsigned char> d_scratch;
    mi355pt_temporal_frame dev[2] = {};
    const mi355pt_temporal_frame* host[2] = {cur, prev};
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        const float* src[6] = {host[k]->film, host[k]->half, k == 0 ? nullptr : host[k]->length, host[k]->position, host[k]->shading_normal, host[k]->hit};
        const DevBuf<float>* d = d_in[k];
        for (int i = 0; i < 6; ++i) HIP_TRY(d_in[k][i].upload(src[i], i == 2 ? np : n));
        dev[k].film = d[0].p; dev[k].half = d[1].p; dev[k].length = d[2].p; dev[k].position = d[3].p; dev[k].shading_normal = d[4].p; dev[k].hit = d[5].p;
    }
    HIP_TRY(d_ids[0].upload(ids_cur, np));
    HIP_TRY(d_ids[1].upload(ids_prev, np));
    HIP_TRY(d_flow.upload(flow, np));
    HIP_TRY(d_film.alloc(n));
    HIP_TRY(d_len.alloc(np));
    HIP_TRY(d_half.alloc_for(out_half, n));
    if (rp) {
        const size_t scratch_bytes = mi355pt_temporal_rectify_scratch_bytes(width, height);
        HIP_TRY(d_scratch.alloc(scratch_bytes));
        rc = mi355pt_temporal_accumulate_rectified_flow_device(&dev[0], spp, prev ? &dev[1] : nullptr, view, width, height, tp, rp, d_scratch.p, scratch_bytes,
                                                               d_ids[0].p, d_ids[1].p, d_flow.p, d_film.p, d_half.p, d_len.p, nullptr);
    } else {
        rc = mi355pt_temporal_accumulate_flow_device(&dev[0], spp, prev ? &dev[1] : nullptr, view, width, height, tp, d_ids[0].p, d_ids[1].p, d_flow.p, d_film.p,
                                                     d_half.p, d_len.p, nullptr);
    }
    if (rc) return rc;
    HIP_TRY(d_film.download(out_film, n));
    HIP_TRY(d_half.download(out_half, n));
    HIP_TRY(d_len.download(out_length, np));
    return MI355PT_OK;
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
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length);
    if (rc) return rc;
    if ((rc = flow_in_check(d_ids_cur, d_ids_prev, d_flow, 16, d_out_film, d_out_half, d_out_length, nullptr))) return rc;
    const TemporalArgs a = temporal_args(spp, view, width, height, tp);
    const TemporalFrameDev dc = frame_dev(*cur);
    if (!prev) {      // the first frame: nothing to reproject
        HIP_TRY(launch_temporal_accumulate(dc, nullptr, a, d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
        return MI355PT_OK;
    }
    HIP_TRY(launch_temporal_accumulate_flow(dc, frame_dev(*prev), a, FlowArgs{d_ids_cur, d_ids_prev, (const FlowPixelDev*)d_flow}, d_out_film, d_out_half,
                                            d_out_length, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                     uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                     const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, out_film, out_half, out_length);
    if (rc) return rc;
    if ((rc = flow_in_check(ids_cur, ids_prev, flow, 1, out_film, out_half, out_length, nullptr))) return rc;
    return flow_accumulate_host(cur, spp, prev, view, width, height, tp, nullptr, ids_cur, ids_prev, flow, out_film, out_half, out_length);
}

int mi355pt_temporal_accumulate_rectified_flow_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                      const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                      const mi355pt_temporal_rectify_params* rp, void* d_scratch, size_t scratch_bytes, const uint32_t* d_ids_cur,
                                                      const uint32_t* d_ids_prev, const mi355pt_flow_pixel* d_flow, float* d_out_film, float* d_out_half,
                                                      float* d_out_length, void* hip_stream) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length);
    if (rc) return rc;
    if ((rc = rectify_params_check(rp))) return rc;
    if ((rc = rectify_scratch_check(cur, prev, width, height, d_scratch, scratch_bytes, d_out_film, d_out_half, d_out_length))) return rc;
    if ((rc = flow_in_check(d_ids_cur, d_ids_prev, d_flow, 16, d_out_film, d_out_half, d_out_length, d_scratch))) return rc;
    const TemporalArgs a = temporal_args(spp, view, width, height, tp);
    const TemporalFrameDev dc = frame_dev(*cur);
    if (!prev) {      // the first frame: nothing to reproject or rectify, the scratch stays as it is
        HIP_TRY(launch_temporal_accumulate(dc, nullptr, a, d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
        return MI355PT_OK;
    }
    HIP_TRY(launch_temporal_rectify_flow(dc, frame_dev(*prev), a, FlowArgs{d_ids_cur, d_ids_prev, (const FlowPixelDev*)d_flow}, rp->radius, rp->gamma, d_scratch,
                                         d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_rectified_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                               const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                               const mi355pt_temporal_rectify_params* rp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                               const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, out_film, out_half, out_length);
    if (rc) return rc;
    if ((rc = rectify_params_check(rp))) return rc;
    if ((rc = flow_in_check(ids_cur, ids_prev, flow, 1, out_film, out_half, out_length, nullptr))) return rc;
    return flow_accumulate_host(cur, spp, prev, view, width, height, tp, rp, ids_cur, ids_prev, flow, out_film, out_half, out_length);
}

}  // extern "C"
