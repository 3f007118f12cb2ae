// The mi355pt_robust.h surface of libmi355pt.so: the defaults, the argument checks, the combination on device and host buffers, the bucket
// renders and the seam-shaped mi355pt_render_robust.  Host C++ only, like api.cpp; the kernel is in pt_kernels_robust.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "api_internal.hpp"

using namespace pt;

namespace {

bool bucket_count_ok(uint32_t k) { return k == 4u || k == 8u || k == 16u || k == 32u; }

// every check of mi355pt_robust_combine_device / mi355pt_robust_combine; host arithmetic only
int combine_check(const float* buckets, uint32_t n_buckets, uint32_t spp_bucket, uint32_t width, uint32_t height, const mi355pt_robust_params* rp, const float* out,
                  const float* out_half, const uint8_t* out_trim) {
    if (!rp || !buckets || !out) return fail(MI355PT_E_INVALID, "robust combine: null params, buckets or output pointer");
    if (rp->mode > MI355PT_ROBUST_GMON) return fail(MI355PT_E_INVALID, "robust combine: unknown mode");
    if (!std::isfinite(rp->gini_scale) || rp->gini_scale < 0.0f) return fail(MI355PT_E_INVALID, "robust combine: gini_scale must be finite and >= 0");
    if (!bucket_count_ok(n_buckets)) return fail(MI355PT_E_INVALID, "robust combine: n_buckets must be 4, 8, 16 or 32");
    if (spp_bucket == 0) return fail(MI355PT_E_INVALID, "robust combine: spp_bucket must be > 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "robust combine: zero width or height");
    if (frame_too_large(width, height)) return fail(MI355PT_E_INVALID, "robust combine: frame too large (width and height up to 2^24, fewer than 2^32 pixels)");
    const size_t pixels = (size_t)width * height, film_bytes = pixels * 3 * sizeof(float);
    const void* outs[3] = {out, out_half, out_trim};
    const size_t out_bytes[3] = {film_bytes, film_bytes, pixels * 2};
    for (int i = 0; i < 3; ++i) {
        if (overlap(outs[i], out_bytes[i], buckets, film_bytes * n_buckets)) return fail(MI355PT_E_INVALID, "robust combine: an output lies inside the bucket films");
        for (int j = i + 1; j < 3; ++j)
            if (overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(MI355PT_E_INVALID, "robust combine: two outputs are equal or overlap");
    }
    return MI355PT_OK;
}

// what mi355pt_render_buckets_device refuses before check_args looks at the scene and the device
int buckets_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t n_buckets, const float* d_buckets) {
    if (!s || !cam || !p || !d_buckets) return fail(MI355PT_E_INVALID, "render buckets: null argument");
    if (!bucket_count_ok(n_buckets)) return fail(MI355PT_E_INVALID, "render buckets: n_buckets must be 4, 8, 16 or 32");
    if (p->spp == 0 || p->spp % n_buckets != 0) return fail(MI355PT_E_INVALID, "render buckets: spp must be a multiple of n_buckets above 0");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "render buckets: collect_stats must be 0 (a bucket is a plain launch)");
    return MI355PT_OK;
}

}  // namespace

extern "C" {

void mi355pt_robust_params_default(mi355pt_robust_params* out) {
    if (!out) return;
    out->mode = MI355PT_ROBUST_GMON; out->gini_scale = 1.0f;
}

int mi355pt_robust_combine_device(const float* d_buckets, uint32_t n_buckets, uint32_t spp_bucket, uint32_t width, uint32_t height, const mi355pt_robust_params* rp,
                                  float* d_out, float* d_out_half, uint8_t* d_out_trim, void* hip_stream) {
    int rc = combine_check(d_buckets, n_buckets, spp_bucket, width, height, rp, d_out, d_out_half, d_out_trim);
    if (rc) return rc;
    RobustArgs a{};
    a.pixels = (uint64_t)width * height; a.spp = (float)spp_bucket; a.inv_spp = (spp_bucket & (spp_bucket - 1u)) == 0u ? 1.0f / a.spp : 0.0f; a.mode = rp->mode; a.gini_scale = rp->gini_scale;
    HIP_TRY(launch_robust_combine(d_buckets, n_buckets, a, d_out, d_out_half, d_out_trim, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_robust_combine(const float* buckets, uint32_t n_buckets, uint32_t spp_bucket, uint32_t width, uint32_t height, const mi355pt_robust_params* rp, float* out,
                           float* out_half, uint8_t* out_trim) {
    int rc = combine_check(buckets, n_buckets, spp_bucket, width, height, rp, out, out_half, out_trim);
    if (rc) return rc;
    const size_t pixels = (size_t)width * height, n = pixels * 3;
    DevBuf<float> d_buckets, d_out, d_half;
    DevBuf<uint8_t> d_trim;
    HIP_TRY(d_buckets.upload(buckets, n * n_buckets));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(d_half.alloc_for(out_half, n));
    HIP_TRY(d_trim.alloc_for(out_trim, pixels * 2));
    if ((rc = mi355pt_robust_combine_device(d_buckets.p, n_buckets, spp_bucket, width, height, rp, d_out.p, d_half.p, d_trim.p, nullptr))) return rc;
    HIP_TRY(d_out.download(out, n));
    HIP_TRY(d_half.download(out_half, n));
    HIP_TRY(d_trim.download(out_trim, pixels * 2));
    return MI355PT_OK;
}

int mi355pt_render_buckets_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t n_buckets, float* d_buckets, void* hip_stream,
                                  mi355pt_stats* stats) {
    int rc = buckets_check(s, cam, p, n_buckets, d_buckets);
    if (rc) return rc;
    if ((rc = check_args(s, cam, p))) return rc;
    const size_t n = (size_t)cam->width * cam->height * 3;
    const uint32_t per = p->spp / n_buckets;
    HIP_TRY(hipMemsetAsync(d_buckets, 0, n * n_buckets * sizeof(float), (hipStream_t)hip_stream));
    double ms = 0.0;
    uint32_t launches = 0;
    for (uint32_t k = 0; k < n_buckets; ++k) {
        mi355pt_stats st;
        if ((rc = render_accum_range(s, cam, p, k * per, (k + 1u) * per, d_buckets + k * n, hip_stream, stats ? &st : nullptr, PathOut{nullptr, nullptr, nullptr, 0u, 0u}))) return rc;
        if (stats) { ms += st.kernel_ms; launches += st.launches; }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms; stats->launches = launches;
    }
    return MI355PT_OK;
}

int mi355pt_render_robust(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t n_buckets, const mi355pt_robust_params* rp,
                          float* out_rgb) {
    int rc = buckets_check(s, cam, p, n_buckets, out_rgb);
    if (rc) return rc;
    if (!rp) return fail(MI355PT_E_INVALID, "render robust: null robust params");
    // (what the combination would refuse, before anything is allocated; its pointer checks concern the buffers made below)
    if (cam->width == 0 || cam->height == 0) return fail(MI355PT_E_INVALID, "render robust: zero width or height");
    if (rp->mode > MI355PT_ROBUST_GMON) return fail(MI355PT_E_INVALID, "render robust: unknown mode");
    if (!std::isfinite(rp->gini_scale) || rp->gini_scale < 0.0f) return fail(MI355PT_E_INVALID, "render robust: gini_scale must be finite and >= 0");
    if ((rc = check_args(s, cam, p))) return rc;
    const size_t n = (size_t)cam->width * cam->height * 3;
    DevBuf<float> d_buckets, d_theta, d_rgb;
    HIP_TRY(d_buckets.alloc(n * n_buckets));
    HIP_TRY(d_theta.alloc(n));
    HIP_TRY(d_rgb.alloc(n));
    if ((rc = mi355pt_render_buckets_device(s, cam, p, n_buckets, d_buckets.p, nullptr, nullptr))) return rc;
    if ((rc = mi355pt_robust_combine_device(d_buckets.p, n_buckets, p->spp / n_buckets, cam->width, cam->height, rp, d_theta.p, nullptr, nullptr, nullptr))) return rc;
    if ((rc = mi355pt_film_resolve_device(d_theta.p, cam->width * cam->height, 1u, d_rgb.p, nullptr))) return rc;
    HIP_TRY(d_rgb.download(out_rgb, n));
    return MI355PT_OK;
}

}  // extern "C"
