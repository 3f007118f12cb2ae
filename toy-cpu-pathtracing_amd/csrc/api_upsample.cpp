// The mi355pt_upsample.h surface of libmi355pt.so: the low camera (host arithmetic), the argument checks and the two entry points of the
// guided half-resolution upsample.  Host C++ only, like api.cpp; the kernel is pt_kernels_upsample.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "api_internal.hpp"

using namespace pt;

namespace {

// every check of mi355pt_upsample_device / mi355pt_upsample; host arithmetic only
int upsample_check(const float* low_film, const float* low_half, uint32_t spp, const mi355pt_upsample_guides* lg, uint32_t spp_albedo_low,
                   const mi355pt_upsample_guides* fg, uint32_t spp_albedo_full, uint32_t width, uint32_t height, const mi355pt_upsample_params* up,
                   const float* out_film, const float* out_half) {
    if (!up || !low_film || !out_film || !lg || !fg) return fail(MI355PT_E_INVALID, "upsample: null params, low film, output film or guides pointer");
    if (!lg->shading_normal || !lg->position || !lg->hit || !fg->shading_normal || !fg->position || !fg->hit)
        return fail(MI355PT_E_INVALID, "upsample: the low and the full guides need their shading_normal, position and hit films");
    if ((lg->albedo != nullptr) != (fg->albedo != nullptr)) return fail(MI355PT_E_INVALID, "upsample: the albedo films of the low and the full guides must both be given or both be NULL");
    if (lg->albedo && (spp_albedo_low == 0 || spp_albedo_full == 0)) return fail(MI355PT_E_INVALID, "upsample: spp_albedo_low and spp_albedo_full must be > 0 with albedo films");
    const bool half = low_half != nullptr;
    if ((out_half != nullptr) != half) return fail(MI355PT_E_INVALID, "upsample: the low half film and the output half film must both be given or both be NULL");
    if (spp == 0 || (half && (spp & 1u) != 0u)) return fail(MI355PT_E_INVALID, "upsample: spp must be > 0, and even with a half film (it holds the first spp / 2 samples)");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "upsample: zero width or height");
    if ((width & 1u) != 0u || (height & 1u) != 0u) return fail(MI355PT_E_INVALID, "upsample: width and height (the FULL size) must be even: the low frame is width / 2 x height / 2");
    if (frame_side_too_large(width, height) || denoise_grid_blocks(width, height) == 0) return fail(MI355PT_E_INVALID, "upsample: frame too large");
    const float fin[4] = {up->pos_tol, up->emitter_tol, up->min_weight, up->albedo_eps};
    for (float v : fin)
        if (!std::isfinite(v)) return fail(MI355PT_E_INVALID, "upsample: pos_tol, emitter_tol, min_weight and albedo_eps must be finite");
    if (!(up->pos_tol > 0.0f && up->min_weight > 0.0f && up->albedo_eps > 0.0f))
        return fail(MI355PT_E_INVALID, "upsample: pos_tol, min_weight and albedo_eps must be > 0 (mi355pt_upsample_params_default fills the struct)");
    if (!(up->emitter_tol >= 0.0f)) return fail(MI355PT_E_INVALID, "upsample: emitter_tol must be >= 0");
    if (!(up->normal_cos >= -1.0f && up->normal_cos <= 1.0f)) return fail(MI355PT_E_INVALID, "upsample: normal_cos must be in [-1, 1]");
    const float* in[10] = {low_film, low_half, lg->albedo, lg->shading_normal, lg->position, lg->hit, fg->albedo, fg->shading_normal, fg->position, fg->hit};
    const float* out[2] = {out_film, out_half};
    for (const float* o : out) {
        if (!o) continue;
        for (const float* q : in)
            if (q == o) return fail(MI355PT_E_INVALID, "upsample: an output must not be one of the inputs");
    }
    if (out_film == out_half) return fail(MI355PT_E_INVALID, "upsample: the two outputs are the same buffer");
    return MI355PT_OK;
}

UpsampleGuidesDev guides_dev(const mi355pt_upsample_guides& g) {
    UpsampleGuidesDev d;
    d.albedo = g.albedo; d.shading_normal = g.shading_normal; d.position = g.position; d.hit = g.hit;
    return d;
}

}  // namespace

extern "C" {

void mi355pt_upsample_params_default(mi355pt_upsample_params* out) {
    if (!out) return;
    out->pos_tol = 0.01f; out->normal_cos = 0.9f; out->emitter_tol = 0.25f; out->min_weight = 0.01f; out->albedo_eps = 0.01f;
}

int mi355pt_upsample_low_camera(const mi355pt_camera* full, mi355pt_camera* low) {
    if (!full || !low) return fail(MI355PT_E_INVALID, "upsample low camera: null argument");
    if (full->width == 0 || full->height == 0 || (full->width & 1u) != 0u || (full->height & 1u) != 0u)
        return fail(MI355PT_E_INVALID, "upsample low camera: width and height must be even and above 0");
    const mi355pt_camera c = *full;      // (full and low may be the same object)
    *low = c;
    low->width = c.width / 2; low->height = c.height / 2;
    return MI355PT_OK;
}

int mi355pt_upsample_device(const float* d_low_film, const float* d_low_half, uint32_t spp, const mi355pt_upsample_guides* lg, uint32_t spp_albedo_low,
                            const mi355pt_upsample_guides* fg, uint32_t spp_albedo_full, uint32_t width, uint32_t height, const mi355pt_upsample_params* up,
                            float* d_out_film, float* d_out_half, void* hip_stream) {
    int rc = upsample_check(d_low_film, d_low_half, spp, lg, spp_albedo_low, fg, spp_albedo_full, width, height, up, d_out_film, d_out_half);
    if (rc) return rc;
    UpsampleArgs a{};
    a.width = width; a.height = height;
    a.spp = (float)spp; a.half_spp = (float)(spp >> 1);
    a.spp_albedo_low = (float)spp_albedo_low; a.spp_albedo_full = (float)spp_albedo_full;
    a.pos_tol = up->pos_tol; a.normal_cos = up->normal_cos; a.emitter_tol = up->emitter_tol; a.min_weight = up->min_weight; a.albedo_eps = up->albedo_eps;
    HIP_TRY(launch_upsample(d_low_film, d_low_half, guides_dev(*lg), guides_dev(*fg), a, d_out_film, d_out_half, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_upsample(const float* low_film, const float* low_half, uint32_t spp, const mi355pt_upsample_guides* lg, uint32_t spp_albedo_low,
                     const mi355pt_upsample_guides* fg, uint32_t spp_albedo_full, uint32_t width, uint32_t height, const mi355pt_upsample_params* up,
                     float* out_film, float* out_half) {
    int rc = upsample_check(low_film, low_half, spp, lg, spp_albedo_low, fg, spp_albedo_full, width, height, up, out_film, out_half);
    if (rc) return rc;
    const size_t n_full = (size_t)width * height * 3, n_low = (size_t)(width / 2) * (height / 2) * 3;
    // the low film, the low half film, the guides of the two resolutions in the order of mi355pt_upsample_guides
    const float* src[10] = {low_film, low_half, lg->albedo, lg->shading_normal, lg->position, lg->hit, fg->albedo, fg->shading_normal, fg->position, fg->hit};
    DevBuf<float> d[10], d_film, d_half;
    for (int i = 0; i < 10; ++i) HIP_TRY(d[i].upload(src[i], i < 6 ? n_low : n_full));
    HIP_TRY(d_film.alloc(n_full));
    HIP_TRY(d_half.alloc_for(out_half, n_full));
    const mi355pt_upsample_guides dl{d[2].p, d[3].p, d[4].p, d[5].p}, df{d[6].p, d[7].p, d[8].p, d[9].p};
    if ((rc = mi355pt_upsample_device(d[0].p, d[1].p, spp, &dl, spp_albedo_low, &df, spp_albedo_full, width, height, up, d_film.p, d_half.p, nullptr))) return rc;
    HIP_TRY(d_film.download(out_film, n_full));
    HIP_TRY(d_half.download(out_half, n_full));
    return MI355PT_OK;
}

}  // extern "C"
