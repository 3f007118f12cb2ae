// The mi355pt_temporal.h and mi355pt_temporal_rectify.h surfaces of libmi355pt.so: the view of a camera pair (host arithmetic), the four
// entry points of the temporal reprojection and of its rectified form — and the one driver behind them and behind the eight carry forms of
// api_motion.cpp and api_flow.cpp (api_internal.hpp): the checks in their one order, the launches with the first-frame rule,
// the host forms' staging.  Host C++ only, like api.cpp; the kernels are pt_kernels_temporal.hip and pt_kernels_temporal_rectify.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "api_internal.hpp"

using namespace pt;

namespace {

bool normalize3(const float v[3], double out[3]) {
    const double x = v[0], y = v[1], z = v[2], l = std::sqrt(x * x + y * y + z * z);
    if (!(std::isfinite(l) && l > 0.0)) return false;
    out[0] = x / l; out[1] = y / l; out[2] = z / l;
    return true;
}

// the checks every form runs first; host arithmetic only
int temporal_check(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                   uint32_t height, const mi355pt_temporal_params* tp, const float* out_film, const float* out_half, const float* out_length) {
    if (!cur || !tp || !out_film || !out_length) return fail(MI355PT_E_INVALID, "temporal: null current frame, params, output film or output length pointer");
    if ((prev == nullptr) != (view == nullptr)) return fail(MI355PT_E_INVALID, "temporal: the previous frame and the view must both be given or both be NULL");
    if (!cur->film || !cur->position || !cur->shading_normal || !cur->hit)
        return fail(MI355PT_E_INVALID, "temporal: the current frame needs its film, position, shading_normal and hit films");
    if (prev && (!prev->film || !prev->length || !prev->position || !prev->shading_normal || !prev->hit))
        return fail(MI355PT_E_INVALID, "temporal: the previous frame needs its film, length, position, shading_normal and hit films");
    const bool half = cur->half != nullptr;
    if ((out_half != nullptr) != half || (prev && (prev->half != nullptr) != half))
        return fail(MI355PT_E_INVALID, "temporal: the half films of the current frame, the previous frame and the output must all be given or all be NULL");
    if (spp == 0 || (half && (spp & 1u) != 0u)) return fail(MI355PT_E_INVALID, "temporal: spp must be > 0, and even with a half film (it holds the first spp / 2 samples)");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "temporal: zero width or height");
    if (frame_side_too_large(width, height) || denoise_grid_blocks(width, height) == 0) return fail(MI355PT_E_INVALID, "temporal: frame too large");
    if (!all_finite_positive({tp->pos_tol, tp->min_weight, tp->max_history}))
        return fail(MI355PT_E_INVALID, "temporal: pos_tol, min_weight and max_history must be finite and > 0 (mi355pt_temporal_params_default fills the struct)");
    if (tp->max_history < 1.0f) return fail(MI355PT_E_INVALID, "temporal: max_history must be >= 1");
    if (!(tp->normal_cos >= -1.0f && tp->normal_cos <= 1.0f)) return fail(MI355PT_E_INVALID, "temporal: normal_cos must be in [-1, 1]");
    const float* in[11] = {cur->film, cur->half, cur->position, cur->shading_normal, cur->hit, prev ? prev->film : nullptr, prev ? prev->half : nullptr,
                           prev ? prev->length : nullptr, prev ? prev->position : nullptr, prev ? prev->shading_normal : nullptr, prev ? prev->hit : nullptr};
    const float* out[3] = {out_film, out_half, out_length};
    for (int i = 0; i < 3; ++i) {
        if (!out[i]) continue;
        for (const float* q : in)
            if (q == out[i]) return fail(MI355PT_E_INVALID, "temporal: an output must not be one of the inputs");
        for (int j = i + 1; j < 3; ++j)
            if (out[j] == out[i]) return fail(MI355PT_E_INVALID, "temporal: two outputs are the same buffer");
    }
    return MI355PT_OK;
}

TemporalFrameDev frame_dev(const mi355pt_temporal_frame& f) {
    TemporalFrameDev d;
    d.film = f.film; d.half = f.half; d.length = f.length; d.position = f.position; d.shading_normal = f.shading_normal; d.hit = f.hit;
    return d;
}

TemporalArgs temporal_args(uint32_t spp, const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp) {
    TemporalArgs a{};
    a.width = width; a.height = height;
    a.spp = (float)spp; a.half_spp = (float)(spp >> 1);
    a.wf = (float)width; a.hf = (float)height;
    if (view) {
        for (int i = 0; i < 3; ++i) a.delta[i] = view->delta[i];
        for (int i = 0; i < 9; ++i) a.rows[i] = view->rows[i];
        a.sx = view->sx; a.sy = view->sy; a.cx = view->cx; a.cy = view->cy;
    }
    a.pos_tol = tp->pos_tol; a.normal_cos = tp->normal_cos; a.min_weight = tp->min_weight; a.max_history = tp->max_history;
    return a;
}

// what mi355pt_temporal_rectify.h adds to temporal_check: the rectification's own parameters ...
int rectify_params_check(const mi355pt_temporal_rectify_params* rp) {
    if (!rp) return fail(MI355PT_E_INVALID, "temporal rectify: null rectify_params pointer");
    if (rp->radius < 1 || rp->radius > 3) return fail(MI355PT_E_INVALID, "temporal rectify: radius must be 1, 2 or 3 (mi355pt_temporal_rectify_params_default fills the struct)");
    if (!all_finite_positive({rp->gamma})) return fail(MI355PT_E_INVALID, "temporal rectify: gamma must be finite and > 0");
    return MI355PT_OK;
}
// ... and the device entry point's scratch
int rectify_scratch_check(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, uint32_t width, uint32_t height, const void* scratch,
                          size_t scratch_bytes, const float* out_film, const float* out_half, const float* out_length) {
    // (not scratch_verdict: this entry point names the alignment before the size)
    if (!scratch) return fail(MI355PT_E_INVALID, "temporal rectify: null scratch pointer");
    if (misaligned(scratch, 16)) return fail(MI355PT_E_INVALID, "temporal rectify: the scratch must be 16-byte aligned");
    const size_t need = mi355pt_temporal_rectify_scratch_bytes(width, height);
    if (need == 0 || scratch_bytes < need) return fail(MI355PT_E_INVALID, "temporal rectify: scratch smaller than mi355pt_temporal_rectify_scratch_bytes(width, height)");
    const void* other[15] = {cur->film, cur->half, cur->length, cur->position, cur->shading_normal, cur->hit, prev ? prev->film : nullptr,
                             prev ? prev->half : nullptr, prev ? prev->length : nullptr, prev ? prev->position : nullptr,
                             prev ? prev->shading_normal : nullptr, prev ? prev->hit : nullptr, out_film, out_half, out_length};
    for (const void* q : other)
        if (q == scratch) return fail(MI355PT_E_INVALID, "temporal rectify: the scratch must not be one of the inputs or outputs");
    return MI355PT_OK;
}

// the checks of a call in their one order; `device`: a _device form, whose scratch is the caller's
int call_check(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect, bool device) {
    int rc = temporal_check(c.cur, c.spp, c.prev, c.view, c.width, c.height, c.tp, c.out_film, c.out_half, c.out_length);
    if (rc) return rc;
    if (rect && (rc = rectify_params_check(rect->rp))) return rc;
    const void* scratch = rect && device ? rect->scratch : nullptr;
    if (rect && device && (rc = rectify_scratch_check(c.cur, c.prev, c.width, c.height, scratch, rect->scratch_bytes, c.out_film, c.out_half, c.out_length))) return rc;
    switch (carry.kind) {
        case TemporalCarry::TABLE: return motion_check(carry, c, scratch);
        case TemporalCarry::FLOW: return flow_in_check(carry, c, scratch);
        case TemporalCarry::NONE: break;
    }
    return MI355PT_OK;
}

// The launches of a checked call whose buffers are all on the device.  The first frame (no previous one) has nothing to reproject or to
// rectify: whatever the form, it is the plain kernel, and a scratch stays as it is.  Otherwise the carry's accumulation, or for a rectified
// form the carry's gather into the scratch and then the one rectifying blend
int run_device(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect, hipStream_t stream) {
    const TemporalArgs a = temporal_args(c.spp, c.view, c.width, c.height, c.tp);
    const TemporalFrameDev dc = frame_dev(*c.cur);
    const TemporalCarryDev cv = carry_dev(carry);
    const TemporalOutsDev outs{c.out_film, c.out_half, c.out_length};
    TemporalFrameDev dp;
    if (c.prev) dp = frame_dev(*c.prev);
    if (!c.prev || !rect) {
        HIP_TRY(launch_temporal_accumulate(dc, c.prev ? &dp : nullptr, a, cv, outs, stream));
        return MI355PT_OK;
    }
    HIP_TRY(launch_temporal_gather(dc, dp, a, cv, rect->scratch, stream));
    HIP_TRY(launch_temporal_rectify_blend(dc, a, rect->rp->radius, rect->rp->gamma, rect->scratch, c.out_film, c.out_half, c.out_length, stream));
    return MI355PT_OK;
}

}  // namespace

int pt::temporal_accumulate_device(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect, void* hip_stream) {
    const int rc = call_check(c, carry, rect, true);
    return rc ? rc : run_device(c, carry, rect, (hipStream_t)hip_stream);
}

// A host form: its own checks (no scratch, no alignment asked), then device copies of the films, of the ids when given and of the table or
// the records, the launches of the device form (rectified: with a scratch of its own) on the null stream, the outputs copied back
int pt::temporal_accumulate_host(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect) {
    const int rc = call_check(c, carry, rect, false);
    if (rc) return rc;
    const size_t np = (size_t)c.width * c.height, n = np * 3;
    // the films of the two frames in the order of mi355pt_temporal_frame (length: W x H; the current frame's is ignored)
    DevBuf<float> d_in[2][6], d_film, d_half, d_len;
    DevBuf<uint32_t> d_ids[2];
    DevBuf<mi355pt_motion_xform> d_table;
    DevBuf<mi355pt_flow_pixel> d_flow;
    DevBuf<unsigned char> d_scratch;
    mi355pt_temporal_frame dev[2] = {};
    const mi355pt_temporal_frame* host[2] = {c.cur, c.prev};
    for (int k = 0; k < 2; ++k) {
        if (!host[k]) continue;
        const float* src[6] = {host[k]->film, host[k]->half, k == 0 ? nullptr : host[k]->length, host[k]->position, host[k]->shading_normal, host[k]->hit};
        const DevBuf<float>* d = d_in[k];
        for (int i = 0; i < 6; ++i) HIP_TRY(d_in[k][i].upload(src[i], i == 2 ? np : n));
        dev[k].film = d[0].p; dev[k].half = d[1].p; dev[k].length = d[2].p; dev[k].position = d[3].p; dev[k].shading_normal = d[4].p; dev[k].hit = d[5].p;
    }
    HIP_TRY(d_ids[0].upload(carry.ids_cur, np));
    HIP_TRY(d_ids[1].upload(carry.ids_prev, np));
    HIP_TRY(d_table.upload(carry.table, carry.n_entries));
    HIP_TRY(d_flow.upload(carry.flow, np));
    HIP_TRY(d_film.alloc(n));
    HIP_TRY(d_len.alloc(np));
    HIP_TRY(d_half.alloc_for(c.out_half, n));
    TemporalRectify d_rect{rect ? rect->rp : nullptr};
    if (rect) {
        d_rect.scratch_bytes = mi355pt_temporal_rectify_scratch_bytes(c.width, c.height);
        HIP_TRY(d_scratch.alloc(d_rect.scratch_bytes));
        d_rect.scratch = d_scratch.p;
    }
    TemporalCarry d_carry = carry;
    d_carry.ids_cur = d_ids[0].p; d_carry.ids_prev = d_ids[1].p; d_carry.table = d_table.p; d_carry.flow = d_flow.p;
    const TemporalCall d_call{&dev[0], c.spp, c.prev ? &dev[1] : nullptr, c.view, c.width, c.height, c.tp, d_film.p, d_half.p, d_len.p};
    const int run = run_device(d_call, d_carry, rect ? &d_rect : nullptr, nullptr);
    if (run) return run;
    HIP_TRY(d_film.download(c.out_film, n));
    HIP_TRY(d_half.download(c.out_half, n));
    HIP_TRY(d_len.download(c.out_length, np));
    return MI355PT_OK;
}

extern "C" {

void mi355pt_temporal_params_default(mi355pt_temporal_params* out) {
    if (!out) return;
    out->pos_tol = 0.01f; out->normal_cos = 0.9f; out->min_weight = 0.01f; out->max_history = 32.0f;
}

int mi355pt_temporal_view_from_cameras(const mi355pt_camera* cur, const mi355pt_camera* prev, mi355pt_temporal_view* out) {
    if (!cur || !prev || !out) return fail(MI355PT_E_INVALID, "temporal view: null argument");
    if (cur->width == 0 || cur->height == 0 || cur->width != prev->width || cur->height != prev->height)
        return fail(MI355PT_E_INVALID, "temporal view: the two cameras must have the same non-zero width and height");
    if (!(cur->fov_deg == prev->fov_deg)) return fail(MI355PT_E_INVALID, "temporal view: the two cameras must have the same fov_deg");
    double f[3], up[3];
    if (!normalize3(prev->direction, f) || !normalize3(prev->up, up)) return fail(MI355PT_E_INVALID, "temporal view: zero direction or up");
    // look_to_rh(direction, up): s = normalize(f x up), u = s x f; the rows of world -> camera are s, u, -f
    const double c[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double cl = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (!(std::isfinite(cl) && cl > 1e-12)) return fail(MI355PT_E_INVALID, "temporal view: direction is parallel to up");
    const double s[3] = {c[0] / cl, c[1] / cl, c[2] / cl};
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    const double w = (double)cur->width, h = (double)cur->height;
    const double scale = std::tan((double)prev->fov_deg * (3.14159265358979323846 / 180.0) / 2.0);
    if (!(std::isfinite(scale) && scale > 0.0)) return fail(MI355PT_E_INVALID, "temporal view: fov_deg must be in (0, 180)");
    for (int i = 0; i < 3; ++i) {
        out->delta[i] = (float)((double)cur->position[i] - (double)prev->position[i]);
        out->rows[i] = (float)s[i]; out->rows[3 + i] = (float)u[i]; out->rows[6 + i] = (float)-f[i];
    }
    out->sx = (float)((w / 2.0) / ((w / h) * scale));
    out->sy = (float)((h / 2.0) / scale);
    out->cx = (float)(w / 2.0);
    out->cy = (float)(h / 2.0);
    return MI355PT_OK;
}

int mi355pt_temporal_accumulate_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                       uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, float* d_out_film, float* d_out_half,
                                       float* d_out_length, void* hip_stream) {
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length}, TemporalCarry{}, nullptr, hip_stream);
}

int mi355pt_temporal_accumulate(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, float* out_film, float* out_half, float* out_length) {
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, TemporalCarry{}, nullptr);
}

/* ---- mi355pt_temporal_rectify.h ---- */
void mi355pt_temporal_rectify_params_default(mi355pt_temporal_rectify_params* out) {
    if (!out) return;
    out->radius = 2; out->gamma = 2.0f;
}

size_t mi355pt_temporal_rectify_scratch_bytes(uint32_t width, uint32_t height) {
    const size_t np = (size_t)width * (size_t)height;
    if (width != 0 && np / width != height) return 0;
    if (np > SIZE_MAX / TEMPORAL_RECTIFY_RECORD_BYTES) return 0;
    return np * TEMPORAL_RECTIFY_RECORD_BYTES;
}

int mi355pt_temporal_accumulate_rectified_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                 const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* tp,
                                                 const mi355pt_temporal_rectify_params* rp, void* d_scratch, size_t scratch_bytes, float* d_out_film,
                                                 float* d_out_half, float* d_out_length, void* hip_stream) {
    const TemporalRectify rect{rp, d_scratch, scratch_bytes};
    return temporal_accumulate_device({cur, spp, prev, view, width, height, tp, d_out_film, d_out_half, d_out_length}, TemporalCarry{}, &rect, hip_stream);
}

int mi355pt_temporal_accumulate_rectified(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                          uint32_t width, uint32_t height, const mi355pt_temporal_params* tp, const mi355pt_temporal_rectify_params* rp,
                                          float* out_film, float* out_half, float* out_length) {
    const TemporalRectify rect{rp};
    return temporal_accumulate_host({cur, spp, prev, view, width, height, tp, out_film, out_half, out_length}, TemporalCarry{}, &rect);
}

}  // extern "C"
