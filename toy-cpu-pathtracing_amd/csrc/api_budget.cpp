// The mi355pt_budget.h surface of libmi355pt.so: the history probe, the budget driver, the pair normalise and the length credit.  Host C++
// only, like api.cpp, whose launches the driver queues (render_accum_range, launch_ranges) exactly as api_adaptive.cpp's does; the pure
// predicates and the budget formula are budget_plan.hpp, the kernels pt_kernels_budget.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "api_internal.hpp"
#include "budget_plan.hpp"

using namespace pt;

namespace {

int budget_check_params(const mi355pt_budget_params* bp) {
    if (!bp) return fail(MI355PT_E_INVALID, "budget: null budget_params pointer");
    switch (budget_params_verdict(bp->base_spp, bp->max_spp, bp->target_history)) {
        case BudgetParams::BASE: return fail(MI355PT_E_INVALID, "budget: base_spp must be a power of two >= 2");
        case BudgetParams::MAX: return fail(MI355PT_E_INVALID, "budget: max_spp must be a power of two >= base_spp");
        case BudgetParams::TARGET: return fail(MI355PT_E_INVALID, "budget: target_history must be finite and >= 1");
        case BudgetParams::OK: break;
    }
    return MI355PT_OK;
}

int budget_check_frame(const char* who, uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, std::string(who) + ": zero width or height");
    if (frame_side_too_large(width, height) || adaptive_tile_count(width, height) == 0u) return fail(MI355PT_E_INVALID, std::string(who) + ": frame too large");
    return MI355PT_OK;
}

// every check of the probe's two forms; host arithmetic only.  `align`: what is asked of the table or the records (16 device, 1 host)
int probe_check(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                const mi355pt_temporal_params* tp, const mi355pt_budget_motion* mo, const mi355pt_budget_params* bp, const float* pred, const float* tile_len,
                const uint32_t* tile_spp, size_t align) {
    if (!cur || !tp || !tile_len || !tile_spp) return fail(MI355PT_E_INVALID, "budget: null current frame, temporal params, tile length or tile count pointer");
    int rc = budget_check_params(bp);
    if (rc) return rc;
    if ((prev == nullptr) != (view == nullptr)) return fail(MI355PT_E_INVALID, "budget: the previous frame and the view must both be given or both be NULL");
    if (!cur->position || !cur->shading_normal || !cur->hit) return fail(MI355PT_E_INVALID, "budget: the current frame needs its position, shading_normal and hit films");
    if (prev && (!prev->length || !prev->position || !prev->shading_normal || !prev->hit))
        return fail(MI355PT_E_INVALID, "budget: the previous frame needs its length, position, shading_normal and hit films");
    if ((rc = budget_check_frame("budget", width, height))) return rc;
    if (!all_finite_positive({tp->pos_tol, tp->min_weight, tp->max_history}))
        return fail(MI355PT_E_INVALID, "budget: pos_tol, min_weight and max_history must be finite and > 0 (mi355pt_temporal_params_default fills the struct)");
    if (tp->max_history < 1.0f) return fail(MI355PT_E_INVALID, "budget: max_history must be >= 1");
    if (!(tp->normal_cos >= -1.0f && tp->normal_cos <= 1.0f)) return fail(MI355PT_E_INVALID, "budget: normal_cos must be in [-1, 1]");
    const void* outs[3] = {pred, tile_len, tile_spp};
    if (mo) {
        switch (budget_carry_verdict(mo->ids_cur, mo->ids_prev, mo->table, mo->n_entries, mo->flow)) {
            case BudgetCarry::BOTH: return fail(MI355PT_E_INVALID, "budget: motion gives both a table and flow records");
            case BudgetCarry::IDS_ALONE: return fail(MI355PT_E_INVALID, "budget: motion gives ids or n_entries without a table or flow records");
            case BudgetCarry::TABLE:
                switch (motion_verdict(mo->ids_cur, mo->ids_prev, mo->table, mo->n_entries, align, outs, 3)) {
                    case Motion::MISSING: return fail(MI355PT_E_INVALID, "budget: the table form needs the current id buffer");
                    case Motion::NO_ENTRIES: return fail(MI355PT_E_INVALID, "budget: n_entries must be > 0 (entry 0 is the static one)");
                    case Motion::MISALIGNED: return fail(MI355PT_E_INVALID, "budget: the motion table must be 16-byte aligned");
                    case Motion::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "budget: an id buffer or the table must not be an output");
                    case Motion::OK: break;
                }
                break;
            case BudgetCarry::FLOW:
                switch (flow_in_verdict(mo->ids_cur, mo->ids_prev, mo->flow, align, outs, 3)) {
                    case FlowIn::MISSING: break;      // (not reached: the form is chosen by the records' presence)
                    case FlowIn::MISALIGNED: return fail(MI355PT_E_INVALID, "budget: the record buffer must be 16-byte aligned");
                    case FlowIn::PREV_IDS_ALONE: return fail(MI355PT_E_INVALID, "budget: the previous frame's ids need the current frame's");
                    case FlowIn::ALIASES_OUTPUT: return fail(MI355PT_E_INVALID, "budget: the records or an id buffer must not be an output");
                    case FlowIn::OK: break;
                }
                break;
            case BudgetCarry::STATIC: break;
        }
    }
    const void* in[7] = {cur->position, cur->shading_normal, cur->hit, prev ? prev->length : nullptr, prev ? prev->position : nullptr,
                         prev ? prev->shading_normal : nullptr, prev ? prev->hit : nullptr};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        for (const void* q : in)
            if (q == outs[i]) return fail(MI355PT_E_INVALID, "budget: an output must not be one of the films that are read");
        for (int j = i + 1; j < 3; ++j)
            if (outs[j] == outs[i]) return fail(MI355PT_E_INVALID, "budget: two outputs are the same buffer");
    }
    return MI355PT_OK;
}

TemporalFrameDev probe_frame_dev(const mi355pt_temporal_frame& f) {
    TemporalFrameDev d;      // film and half stay null: the probe never reads them
    d.length = f.length; d.position = f.position; d.shading_normal = f.shading_normal; d.hit = f.hit;
    return d;
}

// the one launch of a checked probe whose buffers are all on the device
int probe_run(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
              const mi355pt_temporal_params* tp, const mi355pt_budget_motion* mo, const mi355pt_budget_params* bp, float* d_pred, float* d_tile_len,
              uint32_t* d_tile_spp, hipStream_t stream) {
    TemporalArgs a{};
    a.width = width; a.height = height; a.wf = (float)width; a.hf = (float)height;
    if (view) {
        for (int i = 0; i < 3; ++i) a.delta[i] = view->delta[i];
        for (int i = 0; i < 9; ++i) a.rows[i] = view->rows[i];
        a.sx = view->sx; a.sy = view->sy; a.cx = view->cx; a.cy = view->cy;
    }
    a.pos_tol = tp->pos_tol; a.normal_cos = tp->normal_cos; a.min_weight = tp->min_weight; a.max_history = tp->max_history;
    TemporalCarry carry;
    if (mo && (mo->table || mo->flow)) {
        carry.kind = mo->table ? TemporalCarry::TABLE : TemporalCarry::FLOW;
        carry.ids_cur = mo->ids_cur; carry.ids_prev = mo->ids_prev; carry.table = mo->table; carry.n_entries = mo->n_entries; carry.flow = mo->flow;
    }
    const BudgetTilesDev tiles{0u, 0u, bp->base_spp, bp->max_spp, bp->target_history};
    const TemporalFrameDev dc = probe_frame_dev(*cur);
    TemporalFrameDev dp;
    if (prev) dp = probe_frame_dev(*prev);
    HIP_TRY(launch_budget_probe(dc, prev ? &dp : nullptr, a, carry_dev(carry), tiles, d_pred, d_tile_len, d_tile_spp, stream));
    return MI355PT_OK;
}

int pair_check(const float* film, const float* half, const uint32_t* tile_spp, uint32_t width, uint32_t height, const float* out_film, const float* out_half) {
    if (!film || !half || !tile_spp || !out_film || !out_half) return fail(MI355PT_E_INVALID, "pair normalize: null buffer");
    const int rc = budget_check_frame("pair normalize", width, height);
    if (rc) return rc;
    if (out_film == out_half) return fail(MI355PT_E_INVALID, "pair normalize: the two outputs are the same buffer");
    if (out_film == half || out_half == film) return fail(MI355PT_E_INVALID, "pair normalize: an output must not be the other film's input");
    return MI355PT_OK;
}

}  // namespace

extern "C" {

int mi355pt_temporal_budget_device(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                                   uint32_t height, const mi355pt_temporal_params* tp, const mi355pt_budget_motion* mo, const mi355pt_budget_params* bp,
                                   float* d_pred_length, float* d_tile_len, uint32_t* d_tile_spp, void* hip_stream) {
    const int rc = probe_check(cur, prev, view, width, height, tp, mo, bp, d_pred_length, d_tile_len, d_tile_spp, 16);
    return rc ? rc : probe_run(cur, prev, view, width, height, tp, mo, bp, d_pred_length, d_tile_len, d_tile_spp, (hipStream_t)hip_stream);
}

int mi355pt_temporal_budget(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                            uint32_t height, const mi355pt_temporal_params* tp, const mi355pt_budget_motion* mo, const mi355pt_budget_params* bp, float* pred_length,
                            float* tile_len, uint32_t* tile_spp) {
    int rc = probe_check(cur, prev, view, width, height, tp, mo, bp, pred_length, tile_len, tile_spp, 1);
    if (rc) return rc;
    const size_t np = (size_t)width * height, n = np * 3, n_tiles = adaptive_tile_count(width, height);
    // the films the probe reads, in the order length, position, shading_normal, hit (the current frame's length is not read)
    DevBuf<float> d_in[2][4], d_pred, d_len;
    DevBuf<uint32_t> d_ids[2], d_spp;
    DevBuf<mi355pt_motion_xform> d_table;
    DevBuf<mi355pt_flow_pixel> d_flow;
    mi355pt_temporal_frame dev[2] = {};
    const mi355pt_temporal_frame* host[2] = {cur, prev};
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        const float* src[4] = {k == 0 ? nullptr : host[k]->length, host[k]->position, host[k]->shading_normal, host[k]->hit};
        for (int i = 0; i < 4; ++i) HIP_TRY(d_in[k][i].upload(src[i], i == 0 ? np : n));
        dev[k].length = d_in[k][0].p; dev[k].position = d_in[k][1].p; dev[k].shading_normal = d_in[k][2].p; dev[k].hit = d_in[k][3].p;
    }
    mi355pt_budget_motion d_mo{};
    if (mo && prev) {      // (without a previous frame the motion is checked and not read)
        HIP_TRY(d_ids[0].upload(mo->ids_cur, np));
        HIP_TRY(d_ids[1].upload(mo->ids_prev, np));
        HIP_TRY(d_table.upload(mo->table, mo->n_entries));
        HIP_TRY(d_flow.upload(mo->flow, np));
        d_mo.ids_cur = d_ids[0].p; d_mo.ids_prev = d_ids[1].p; d_mo.table = d_table.p; d_mo.n_entries = mo->n_entries; d_mo.flow = d_flow.p;
    }
    HIP_TRY(d_pred.alloc_for(pred_length, np));
    HIP_TRY(d_len.alloc(n_tiles));
    HIP_TRY(d_spp.alloc(n_tiles));
    if ((rc = probe_run(&dev[0], prev ? &dev[1] : nullptr, view, width, height, tp, &d_mo, bp, d_pred.p, d_len.p, d_spp.p, nullptr))) return rc;
    HIP_TRY(d_pred.download(pred_length, np));
    HIP_TRY(d_len.download(tile_len, n_tiles));
    HIP_TRY(d_spp.download(tile_spp, n_tiles));
    return MI355PT_OK;
}

int mi355pt_render_budget_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const mi355pt_budget_params* bp,
                                 const uint32_t* d_tile_spp, float* d_film, float* d_half, uint32_t* d_list, void* d_scratch, size_t scratch_bytes,
                                 void* hip_stream, mi355pt_adaptive_result* result) {
    int rc = check_tiles_args(s, cam, p);
    if (rc) return rc;
    if ((rc = budget_check_params(bp))) return rc;
    if (p->spp != bp->max_spp) return fail(MI355PT_E_INVALID, "budget: spp must equal max_spp (it fixes the Sobol sequence of every range)");
    if (!d_tile_spp || !d_film || !d_half || !d_list) return fail(MI355PT_E_INVALID, "budget: null buffer");
    if (d_film == d_half) return fail(MI355PT_E_INVALID, "budget: the film and the half film are the same buffer");
    const uint32_t W = cam->width, H = cam->height, n_tiles = adaptive_tile_count(W, H), tiles_x = (W + 7u) / 8u;
    const Scratch sv = scratch_verdict(d_scratch, scratch_bytes, adaptive_scratch_bytes(W, H), 4);
    if (sv == Scratch::MISSING || sv == Scratch::TOO_SMALL) return fail(MI355PT_E_INVALID, "budget: scratch missing or smaller than mi355pt_adaptive_scratch_bytes");
    if (sv == Scratch::MISALIGNED) return fail(MI355PT_E_INVALID, "budget: scratch is not 4-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint32_t base = bp->base_spp, max_spp = bp->max_spp;
    const size_t film_bytes = (size_t)W * H * 3 * sizeof(float);
    uint32_t* d_count = (uint32_t*)((char*)d_scratch + adaptive_scratch_bytes(W, H) - 16u);     // the scratch's last 16 bytes
    const PathOut no_log{nullptr, nullptr, nullptr, 0u, 0u};
    // 1 - 4: every tile at base_spp, H = [0, base / 2), F = [0, base)
    HIP_TRY(hipMemsetAsync(d_film, 0, film_bytes, stream));
    HIP_TRY(hipMemsetAsync(d_half, 0, film_bytes, stream));
    if ((rc = render_accum_range(s, cam, p, 0u, base / 2u, d_half, hip_stream, nullptr, no_log))) return rc;
    HIP_TRY(hipMemcpyAsync(d_film, d_half, film_bytes, hipMemcpyDeviceToDevice, stream));
    if ((rc = render_accum_range(s, cam, p, base / 2u, base, d_film, hip_stream, nullptr, no_log))) return rc;
    // 5: select (H := F on the tiles that go on), count, the listed tiles' next samples
    uint32_t passes = 0;
    for (uint32_t level = base; level < max_spp; level *= 2u) {
        HIP_TRY(launch_budget_select(d_film, d_half, W, H, d_tile_spp, level, base, max_spp, d_scratch, d_list, d_count, stream));
        ++passes;
        uint32_t count = 0;
        HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (count == 0u) break;
        if (count > n_tiles) return fail(MI355PT_E_DEVICE, "budget: the select pass returned more tiles than the frame has");
        if ((rc = launch_ranges(s, cam, p, level, 2u * level, d_film, stream, nullptr, d_list, count))) return rc;
    }
    if (result) {
        std::vector<uint32_t> spp(n_tiles);
        HIP_TRY(hipMemcpyAsync(spp.data(), d_tile_spp, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        result->passes = passes; result->tiles_at_max = 0; result->total_samples = 0;
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const uint32_t tw = std::min(8u, W - (t % tiles_x) * 8u), th = std::min(8u, H - (t / tiles_x) * 8u), n = budget_rendered(spp[t], base, max_spp);
            result->total_samples += (uint64_t)n * tw * th;
            result->tiles_at_max += n == max_spp ? 1u : 0u;
        }
    }
    return MI355PT_OK;
}

int mi355pt_film_pair_normalize_tiles_device(const float* d_film, const float* d_half, const uint32_t* d_tile_spp, uint32_t width, uint32_t height,
                                             float* d_out_film, float* d_out_half, void* hip_stream) {
    const int rc = pair_check(d_film, d_half, d_tile_spp, width, height, d_out_film, d_out_half);
    if (rc) return rc;
    HIP_TRY(launch_pair_normalize_tiles(d_film, d_half, d_tile_spp, width, height, d_out_film, d_out_half, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_film_pair_normalize_tiles(const float* film, const float* half, const uint32_t* tile_spp, uint32_t width, uint32_t height, float* out_film,
                                      float* out_half) {
    const int rc = pair_check(film, half, tile_spp, width, height, out_film, out_half);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3, n_tiles = adaptive_tile_count(width, height);
    DevBuf<float> d_film, d_half;
    DevBuf<uint32_t> d_spp;
    HIP_TRY(d_film.upload(film, n)); HIP_TRY(d_half.upload(half, n)); HIP_TRY(d_spp.upload(tile_spp, n_tiles));
    HIP_TRY(launch_pair_normalize_tiles(d_film.p, d_half.p, d_spp.p, width, height, d_film.p, d_half.p, nullptr));
    HIP_TRY(d_film.download(out_film, n));
    HIP_TRY(d_half.download(out_half, n));
    return MI355PT_OK;
}

int mi355pt_temporal_length_credit_device(float* d_length, const uint32_t* d_tile_spp, uint32_t base_spp, float max_history, uint32_t width, uint32_t height,
                                          void* hip_stream) {
    if (!d_length || !d_tile_spp) return fail(MI355PT_E_INVALID, "length credit: null buffer");
    const int rc = budget_check_frame("length credit", width, height);
    if (rc) return rc;
    if (base_spp < 2u || !budget_pow2(base_spp)) return fail(MI355PT_E_INVALID, "length credit: base_spp must be a power of two >= 2");
    if (!(std::isfinite(max_history) && max_history >= 1.0f)) return fail(MI355PT_E_INVALID, "length credit: max_history must be finite and >= 1");
    HIP_TRY(launch_length_credit(d_length, d_tile_spp, base_spp, max_history, width, height, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

}  // extern "C"
