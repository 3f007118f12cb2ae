// The mi355pt_denoise.h surface of libmi355pt.so — the defaults, the scratch size, the argument checks and the two entry points of the
// AOV-guided denoiser — and the mi355pt_denoise_var.h surface, the variance-guided denoiser's, of the same shape.  Host C++ only, like
// api.cpp; the kernels are pt_kernels_denoise.hip and pt_kernels_denoise_var.hip.
#include "api_internal.hpp"

using namespace pt;

// every check of mi355pt_denoise_device / mi355pt_denoise that does not concern the scratch; host arithmetic only
static int denoise_check(const float* beauty, uint32_t spp_b, const float* albedo, uint32_t spp_a, const float* normal, uint32_t spp_n, uint32_t width,
                         uint32_t height, const mi355pt_denoise_params* dp, const float* out) {
    if (!beauty || !out || !dp) return fail(MI355PT_E_INVALID, "denoise: null beauty, output or params pointer");
    if (dp->levels < 1 || dp->levels > 8) return fail(MI355PT_E_INVALID, "denoise: levels must be 1 .. 8 (mi355pt_denoise_params_default fills the struct)");
    if (!all_finite_positive({dp->sigma_color, dp->sigma_normal, dp->sigma_albedo, dp->albedo_eps}))
        return fail(MI355PT_E_INVALID, "denoise: sigma_color, sigma_normal, sigma_albedo and albedo_eps must be finite and > 0");
    if (spp_b == 0 || (albedo && spp_a == 0) || (normal && spp_n == 0)) return fail(MI355PT_E_INVALID, "denoise: spp of a given buffer is 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "denoise: zero width or height");
    if (denoise_grid_blocks(width, height) == 0 || denoise_scratch_bytes(width, height) == 0) return fail(MI355PT_E_INVALID, "denoise: frame too large");
    if (out == beauty || out == albedo || out == normal) return fail(MI355PT_E_INVALID, "denoise: the output must not be one of the inputs");
    return MI355PT_OK;
}

// every check of mi355pt_denoise_var_device / mi355pt_denoise_var that does not concern the scratch; host arithmetic only
static int denoise_var_check(const float* beauty, const float* half, uint32_t spp_b, const uint32_t* tile_spp, const float* albedo, uint32_t spp_a,
                             const float* normal, uint32_t spp_n, uint32_t width, uint32_t height, const mi355pt_denoise_var_params* dp, const float* out) {
    if (!beauty || !half || !out || !dp) return fail(MI355PT_E_INVALID, "denoise_var: null beauty, half film, output or params pointer");
    if (dp->levels < 1 || dp->levels > 8) return fail(MI355PT_E_INVALID, "denoise_var: levels must be 1 .. 8 (mi355pt_denoise_var_params_default fills the struct)");
    if (!all_finite_positive({dp->sigma_lum, dp->sigma_normal, dp->sigma_albedo, dp->albedo_eps, dp->lum_eps}))
        return fail(MI355PT_E_INVALID, "denoise_var: sigma_lum, sigma_normal, sigma_albedo, albedo_eps and lum_eps must be finite and > 0");
    if (!tile_spp && (spp_b == 0 || (spp_b & 1u) != 0u)) return fail(MI355PT_E_INVALID, "denoise_var: spp_beauty must be even and > 0 (the half film holds the first spp_beauty / 2 samples)");
    if (tile_spp && spp_b != 0) return fail(MI355PT_E_INVALID, "denoise_var: spp_beauty must be 0 when tile counts are given");
    if ((albedo && spp_a == 0) || (normal && spp_n == 0)) return fail(MI355PT_E_INVALID, "denoise_var: spp of a given buffer is 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "denoise_var: zero width or height");
    if (denoise_grid_blocks(width, height) == 0 || denoise_var_scratch_bytes(width, height) == 0) return fail(MI355PT_E_INVALID, "denoise_var: frame too large");
    if (out == beauty || out == half || out == albedo || out == normal || (const void*)out == (const void*)tile_spp)
        return fail(MI355PT_E_INVALID, "denoise_var: the output must not be one of the inputs");
    return MI355PT_OK;
}

extern "C" {

void mi355pt_denoise_params_default(mi355pt_denoise_params* out) {
    if (!out) return;
    out->levels = 5; out->sigma_color = 1.0f; out->sigma_normal = 0.5f; out->sigma_albedo = 0.3f; out->albedo_eps = 0.01f;
}
size_t mi355pt_denoise_scratch_bytes(uint32_t width, uint32_t height) { return denoise_scratch_bytes(width, height); }

int mi355pt_denoise_device(const float* d_beauty, uint32_t spp_b, const float* d_albedo, uint32_t spp_a, const float* d_normal, uint32_t spp_n,
                           uint32_t width, uint32_t height, const mi355pt_denoise_params* dp, void* d_scratch, size_t scratch_bytes, float* d_out,
                           void* hip_stream) {
    int rc = denoise_check(d_beauty, spp_b, d_albedo, spp_a, d_normal, spp_n, width, height, dp, d_out);
    if (rc) return rc;
    const Scratch sv = scratch_verdict(d_scratch, scratch_bytes, denoise_scratch_bytes(width, height), 16);
    if (sv == Scratch::MISSING || sv == Scratch::TOO_SMALL) return fail(MI355PT_E_INVALID, "denoise: scratch missing or smaller than mi355pt_denoise_scratch_bytes");
    if (sv == Scratch::MISALIGNED) return fail(MI355PT_E_INVALID, "denoise: scratch is not 16-byte aligned");
    HIP_TRY(launch_denoise(d_beauty, spp_b, d_albedo, spp_a, d_normal, spp_n, width, height, dp->levels, dp->sigma_color, dp->sigma_normal,
                           dp->sigma_albedo, dp->albedo_eps, d_scratch, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_denoise(const float* beauty, uint32_t spp_b, const float* albedo, uint32_t spp_a, const float* normal, uint32_t spp_n, uint32_t width,
                    uint32_t height, const mi355pt_denoise_params* dp, float* out) {
    int rc = denoise_check(beauty, spp_b, albedo, spp_a, normal, spp_n, width, height, dp, out);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3, scratch_bytes = denoise_scratch_bytes(width, height);
    DevBuf<float> d_b, d_a, d_n, d_out;
    DevBuf<unsigned char> d_scratch;
    HIP_TRY(d_b.upload(beauty, n));
    HIP_TRY(d_a.upload(albedo, n));
    HIP_TRY(d_n.upload(normal, n));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    if ((rc = mi355pt_denoise_device(d_b.p, spp_b, d_a.p, spp_a, d_n.p, spp_n, width, height, dp, d_scratch.p, scratch_bytes, d_out.p, nullptr))) return rc;
    HIP_TRY(d_out.download(out, n));
    return MI355PT_OK;
}

/* ---- mi355pt_denoise_var.h ---- */
void mi355pt_denoise_var_params_default(mi355pt_denoise_var_params* out) {
    if (!out) return;
    out->levels = 5; out->sigma_lum = 4.0f; out->sigma_normal = 0.5f; out->sigma_albedo = 0.3f; out->albedo_eps = 0.01f; out->lum_eps = 1e-4f;
}
size_t mi355pt_denoise_var_scratch_bytes(uint32_t width, uint32_t height) { return denoise_var_scratch_bytes(width, height); }

int mi355pt_denoise_var_device(const float* d_beauty, const float* d_half, uint32_t spp_b, const uint32_t* d_tile_spp, const float* d_albedo, uint32_t spp_a,
                               const float* d_normal, uint32_t spp_n, uint32_t width, uint32_t height, const mi355pt_denoise_var_params* dp, void* d_scratch,
                               size_t scratch_bytes, float* d_out, void* hip_stream) {
    int rc = denoise_var_check(d_beauty, d_half, spp_b, d_tile_spp, d_albedo, spp_a, d_normal, spp_n, width, height, dp, d_out);
    if (rc) return rc;
    const Scratch sv = scratch_verdict(d_scratch, scratch_bytes, denoise_var_scratch_bytes(width, height), 16);
    if (sv == Scratch::MISSING || sv == Scratch::TOO_SMALL) return fail(MI355PT_E_INVALID, "denoise_var: scratch missing or smaller than mi355pt_denoise_var_scratch_bytes");
    if (sv == Scratch::MISALIGNED) return fail(MI355PT_E_INVALID, "denoise_var: scratch is not 16-byte aligned");
    HIP_TRY(launch_denoise_var(d_beauty, d_half, spp_b, d_tile_spp, d_albedo, spp_a, d_normal, spp_n, width, height, dp->levels, dp->sigma_lum, dp->sigma_normal,
                               dp->sigma_albedo, dp->albedo_eps, dp->lum_eps, d_scratch, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_denoise_var(const float* beauty, const float* half_film, uint32_t spp_b, const uint32_t* tile_spp, const float* albedo, uint32_t spp_a,
                        const float* normal, uint32_t spp_n, uint32_t width, uint32_t height, const mi355pt_denoise_var_params* dp, float* out) {
    int rc = denoise_var_check(beauty, half_film, spp_b, tile_spp, albedo, spp_a, normal, spp_n, width, height, dp, out);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3, scratch_bytes = denoise_var_scratch_bytes(width, height);
    const size_t n_tiles = (size_t)((width + 7u) / 8u) * ((height + 7u) / 8u);
    DevBuf<float> d_b, d_h, d_a, d_n, d_out;
    DevBuf<uint32_t> d_t;
    DevBuf<unsigned char> d_scratch;
    HIP_TRY(d_b.upload(beauty, n));
    HIP_TRY(d_h.upload(half_film, n));
    HIP_TRY(d_t.upload(tile_spp, n_tiles));
    HIP_TRY(d_a.upload(albedo, n));
    HIP_TRY(d_n.upload(normal, n));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    if ((rc = mi355pt_denoise_var_device(d_b.p, d_h.p, spp_b, d_t.p, d_a.p, spp_a, d_n.p, spp_n, width, height, dp, d_scratch.p, scratch_bytes, d_out.p, nullptr)))
        return rc;
    HIP_TRY(d_out.download(out, n));
    return MI355PT_OK;
}

}  // extern "C"
