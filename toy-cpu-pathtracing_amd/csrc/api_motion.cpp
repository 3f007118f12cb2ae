// The mi355pt_motion.h surface of libmi355pt.so: the ID pass, the motion table (host arithmetic, motion_plan.hpp) and the four table forms
// of the temporal accumulation: single calls of api_temporal.cpp's driver with a table carry, whose own check is here.  Host C++ only, like
// api.cpp, whose launch context and timed launch the ID pass uses; the ID pass's kernel is in pt_kernels_ids.hip.
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

// what mi355pt_motion.h adds to temporal_check (and, with a scratch, to the rectified form's checks)
int pt::motion_check(const TemporalCarry& carry, const TemporalCall& c, const void* scratch) {
    const void* outs[4] = {c.out_film, c.out_half, c.out_length, scratch};
    switch (motion_verdict(carry.ids_cur, carry.ids_prev, carry.table, carry.n_entries, carry.align, outs, 4)) {
        case Motion::MISSING: return fail(MI355PT_E_INVALID, "temporal motion: null current id buffer or motion table");
        case Motion::NO_ENTRIES: return fail(MI355PT_E_INVALID, "temporal motion: n_entries must be > 0 (entry 0 is the static one)");
        case Motion::MISALIGNED: return fail(MI355PT_E_INVALID, "temporal motion: the motion table must be 16-byte aligned");
        case Motion::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "temporal motion: an id buffer or the table must not be an output or the scratch");
        case Motion::OK: break;
    }
    return MI355PT_OK;
}

namespace {

TemporalCarry table_carry(const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_motion_xform* table, uint32_t n_entries, size_t align) {
    TemporalCarry carry;
    carry.kind = TemporalCarry::TABLE; carry.ids_cur = ids_cur; carry.ids_prev = ids_prev; carry.table = table; carry.n_entries = n_entries; carry.align = align;
    return carry;
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
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length},
                                      table_carry(d_ids_cur, d_ids_prev, d_table, n_entries, 16), nullptr, hip_stream);
}

int mi355pt_temporal_accumulate_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                       uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                       const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film, float* out_half, float* out_length) {
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, table_carry(ids_cur, ids_prev, table, n_entries, 1),
                                    nullptr);
}

int mi355pt_temporal_accumulate_rectified_motion_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                        const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                        const mi355pt_temporal_rectify_params* rp, void* d_scratch, size_t scratch_bytes,
                                                        const uint32_t* d_ids_cur, const uint32_t* d_ids_prev, const mi355pt_motion_xform* d_table,
                                                        uint32_t n_entries, float* d_out_film, float* d_out_half, float* d_out_length, void* hip_stream) {
    const TemporalRectify rect{rp, d_scratch, scratch_bytes};
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length},
                                      table_carry(d_ids_cur, d_ids_prev, d_table, n_entries, 16), &rect, hip_stream);
}

int mi355pt_temporal_accumulate_rectified_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                 const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                 const mi355pt_temporal_rectify_params* rp, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                                 const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film, float* out_half, float* out_length) {
    const TemporalRectify rect{rp};
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, table_carry(ids_cur, ids_prev, table, n_entries, 1),
                                    &rect);
}

}  // extern "C"
