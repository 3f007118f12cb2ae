// The mi355pt_motion.h surface of libmi355pt.so: the ID pass, the motion table (host arithmetic, motion_plan.hpp) and the motion-aware
// twins of the temporal accumulation and of its rectified form, which run api_temporal.cpp's checks and add their own.  Host C++ only, like
// api.cpp, whose launch context and timed launch the ID pass uses; the kernels are in pt_kernels_ids.hip, pt_kernels_temporal.hip and
// pt_kernels_temporal_rectify.hip.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "api_internal.hpp"
#include "motion_plan.hpp"

using namespace pt;

static_assert(sizeof(mi355pt_motion_xform) == sizeof(MotionXform) && sizeof(mi355pt_motion_xform) == sizeof(MotionXformDev), "one layout of a motion record");

// every check of the two ID entry points (and, with its records in the place of the ids, of the flow pass: api_flow.cpp); host memory only
int pt::ids_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const void* ids) {
    if (!ids) return fail(MI355PT_E_INVALID, "ids: null id buffer");
    if (!s || !cam || !p) return fail(MI355PT_E_INVALID, "null argument");
    if (cam->width == 0 || cam->height == 0) return fail(MI355PT_E_INVALID, "ids: zero-sized frame");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "the ID pass has no instrumented kernel: collect_stats must be 0");
    return check_args(s, cam, p, true);
}

// The ID launch's shape: the G-buffer pass's (api_gbuffer.cpp plan_gbuffer) for one sample — the AOV plan with the work item pinned to a
// whole 8x8 tile, one pixel per lane
LaunchPlan pt::plan_ids(const mi355pt_camera* cam, const mi355pt_params* p, int waves) {
    LaunchPlan plan = plan_launch(cam, p, 0u, 1u, waves, true);
    DevParams& dp = plan.params;
    dp.block_log2 = 3u; dp.sample_prefix_digits = 0u;
    dp.n_work = plan.n_tiles * dp.chunks;                      // (chunks == 1)
    plan.grid = (int)std::min<uint32_t>(dp.n_work, (uint32_t)waves);
    return plan;
}

namespace {

// what mi355pt_motion.h adds to temporal_check (and, with a scratch, to the rectified form's checks)
int motion_check(const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_motion_xform* table, uint32_t n_entries, size_t table_align,
                 const void* out_film, const void* out_half, const void* out_length, const void* scratch) {
    const void* outs[4] = {out_film, out_half, out_length, scratch};
    switch (motion_verdict(ids_cur, ids_prev, table, n_entries, table_align, outs, 4)) {
        case Motion::MISSING: return fail(MI355PT_E_INVALID, "temporal motion: null current id buffer or motion table");
        case Motion::NO_ENTRIES: return fail(MI355PT_E_INVALID, "temporal motion: n_entries must be > 0 (entry 0 is the static one)");
        case Motion::MISALIGNED: return fail(MI355PT_E_INVALID, "temporal motion: the motion table must be 16-byte aligned");
        case Motion::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "temporal motion: an id buffer or the table must not be an output or the scratch");
        case Motion::OK: break;
    }
    return MI355PT_OK;
}

// the two host-buffer entry points, after api_temporal.cpp's temporal_accumulate_host: device copies of the films, the ids and the table,
// the device entry point (rectified when rp is given, with a scratch of its own) on the default stream, the outputs copied back.  Every
// argument has been checked.
int motion_accumulate_host(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                           uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const mi355pt_temporal_rectify_params* rp,
                           const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film,
                           float* out_half, float* out_length) {
    int rc = MI355PT_OK;
    const size_t np = (size_t)width * height, n = np * 3;
    DevBuf<float> d_in[2][6], d_film, d_half, d_len;
    DevBuf<uint32_t> d_ids[2];
    DevBuf<mi355pt_motion_xform> d_table;
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
    HIP_TRY(d_table.upload(table, n_entries));
    HIP_TRY(d_film.alloc(n));
    HIP_TRY(d_len.alloc(np));
    HIP_TRY(d_half.alloc_for(out_half, n));
    if (rp) {
        const size_t scratch_bytes = mi355pt_temporal_rectify_scratch_bytes(width, height);
        HIP_TRY(d_scratch.alloc(scratch_bytes));
        rc = mi355pt_temporal_accumulate_rectified_motion_device(&dev[0], spp, prev ? &dev[1] : nullptr, view, width, height, tp, rp, d_scratch.p, scratch_bytes,
                                                                 d_ids[0].p, d_ids[1].p, d_table.p, n_entries, d_film.p, d_half.p, d_len.p, nullptr);
    } else {
        rc = mi355pt_temporal_accumulate_motion_device(&dev[0], spp, prev ? &dev[1] : nullptr, view, width, height, tp, d_ids[0].p, d_ids[1].p, d_table.p,
                                                       n_entries, d_film.p, d_half.p, d_len.p, nullptr);
    }
    if (rc) return rc;
    HIP_TRY(d_film.download(out_film, n));
    HIP_TRY(d_half.download(out_half, n));
    HIP_TRY(d_len.download(out_length, np));
    return MI355PT_OK;
}

MotionArgs motion_args(const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_motion_xform* table, uint32_t n_entries) {
    return MotionArgs{ids_cur, ids_prev, (const MotionXformDev*)table, n_entries - 1u};
}

}  // namespace

extern "C" {

int mi355pt_render_ids_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t* d_ids, void* hip_stream,
                              mi355pt_stats* stats) {
    int rc = ids_check(s, cam, p, d_ids);
    if (rc) return rc;
    if (shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) == 0) return MI355PT_OK;
    LaunchCtx* lc; int slot;
    if ((rc = get_launch_ctx(s, p->seed, &lc, &slot))) return rc;
    if (lc->device != s->impl.device) return fail(MI355PT_E_DEVICE, "launch context and scene live on different devices");
    if (!lc->ids_waves) lc->ids_waves = query_resident_waves_ids();
    const DevCamera dc = make_camera(cam);
    LaunchPlan plan = plan_ids(cam, p, lc->ids_waves);
    plan.params.stats_mode = 0u;
    const hipStream_t stream = (hipStream_t)hip_stream;
    return timed_launch(lc, slot, stream, stats, true, [&](unsigned* d_counter, DevStats* d_stats) {
        HIP_TRY(launch_ids(s->impl.dev, dc, plan.params, d_ids, d_counter, stats ? d_stats : nullptr, plan.grid, stream));
        return (int)MI355PT_OK;
    });
}

int mi355pt_render_ids(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t* ids, mi355pt_stats* stats) {
    int rc = ids_check(s, cam, p, ids);
    if (rc) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    DevBuf<uint32_t> d_ids;
    HIP_TRY(d_ids.alloc(np));
    HIP_TRY(hipMemset(d_ids.p, 0, np * sizeof(uint32_t)));
    if ((rc = mi355pt_render_ids_device(s, cam, p, d_ids.p, nullptr, stats))) return rc;
    HIP_TRY(d_ids.download(ids, np));
    return MI355PT_OK;
}

int mi355pt_motion_table(const mi355pt_camera* cur_cam, const mi355pt_camera* prev_cam, const float* l2w_cur, const float* l2w_prev, uint32_t n,
                         mi355pt_motion_xform* out) {
    if (!cur_cam || !prev_cam || !l2w_cur || !l2w_prev || !out) return fail(MI355PT_E_INVALID, "motion table: null argument");
    if (n == 0) return fail(MI355PT_E_INVALID, "motion table: no instances (n == 0)");
    if (!motion_table(cur_cam->position, prev_cam->position, l2w_cur, l2w_prev, n, (MotionXform*)out))
        return fail(MI355PT_E_INVALID, "motion table: non-finite or singular instance transform");
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_motion_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                              uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* d_ids_cur,
                                              const uint32_t* d_ids_prev, const mi355pt_motion_xform* d_table, uint32_t n_entries, float* d_out_film,
                                              float* d_out_half, float* d_out_length, void* hip_stream) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length);
    if (rc) return rc;
    if ((rc = motion_check(d_ids_cur, d_ids_prev, d_table, n_entries, 16, d_out_film, d_out_half, d_out_length, nullptr))) return rc;
    const TemporalArgs a = temporal_args(spp, view, width, height, tp);
    const TemporalFrameDev dc = frame_dev(*cur);
    if (!prev) {      // the first frame: nothing to reproject
        HIP_TRY(launch_temporal_accumulate(dc, nullptr, a, d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
        return MI355PT_OK;
    }
    HIP_TRY(launch_temporal_accumulate_motion(dc, frame_dev(*prev), a, motion_args(d_ids_cur, d_ids_prev, d_table, n_entries), d_out_film, d_out_half,
                                              d_out_length, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                       uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                       const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film, float* out_half, float* out_length) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, out_film, out_half, out_length);
    if (rc) return rc;
    if ((rc = motion_check(ids_cur, ids_prev, table, n_entries, 1, out_film, out_half, out_length, nullptr))) return rc;
    return motion_accumulate_host(cur, spp, prev, view, width, height, tp, nullptr, ids_cur, ids_prev, table, n_entries, out_film, out_half, out_length);
}

int mi355pt_temporal_accumulate_rectified_motion_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                        const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                        const mi355pt_temporal_rectify_params* rp, void* d_scratch, size_t scratch_bytes,
                                                        const uint32_t* d_ids_cur, const uint32_t* d_ids_prev, const mi355pt_motion_xform* d_table,
                                                        uint32_t n_entries, float* d_out_film, float* d_out_half, float* d_out_length, void* hip_stream) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length);
    if (rc) return rc;
    if ((rc = rectify_params_check(rp))) return rc;
    if ((rc = rectify_scratch_check(cur, prev, width, height, d_scratch, scratch_bytes, d_out_film, d_out_half, d_out_length))) return rc;
    if ((rc = motion_check(d_ids_cur, d_ids_prev, d_table, n_entries, 16, d_out_film, d_out_half, d_out_length, d_scratch))) return rc;
    const TemporalArgs a = temporal_args(spp, view, width, height, tp);
    const TemporalFrameDev dc = frame_dev(*cur);
    if (!prev) {      // the first frame: nothing to reproject or rectify, the scratch stays as it is
        HIP_TRY(launch_temporal_accumulate(dc, nullptr, a, d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
        return MI355PT_OK;
    }
    HIP_TRY(launch_temporal_rectify_motion(dc, frame_dev(*prev), a, motion_args(d_ids_cur, d_ids_prev, d_table, n_entries), rp->radius, rp->gamma, d_scratch,
                                           d_out_film, d_out_half, d_out_length, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_rectified_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                 const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                 const mi355pt_temporal_rectify_params* rp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                                 const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film, float* out_half, float* out_length) {
    int rc = temporal_check(cur, spp, prev, view, width, height, tp, out_film, out_half, out_length);
    if (rc) return rc;
    if ((rc = rectify_params_check(rp))) return rc;
    if ((rc = motion_check(ids_cur, ids_prev, table, n_entries, 1, out_film, out_half, out_length, nullptr))) return rc;
    return motion_accumulate_host(cur, spp, prev, view, width, height, tp, rp, ids_cur, ids_prev, table, n_entries, out_film, out_half, out_length);
}

}  // extern "C"
