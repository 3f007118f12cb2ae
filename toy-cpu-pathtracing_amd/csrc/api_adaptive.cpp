// The mi355pt_adaptive.h surface of libmi355pt.so: the scratch size, the argument checks, the noise step, the per-tile normalisation and the
// two drivers of adaptive sampling.  Host C++ only, like api.cpp, whose launches the drivers queue (render_accum_range, launch_ranges); the
// kernels are in pt_kernels_adaptive.hip.
#include "api_internal.hpp"

using namespace pt;

static int adaptive_check_params(const mi355pt_adaptive_params* ap) {
    if (!ap) return fail(MI355PT_E_INVALID, "adaptive: null params pointer");
    if (!all_finite_positive({ap->threshold})) return fail(MI355PT_E_INVALID, "adaptive: threshold must be finite and > 0 (it has no default)");
    if (!all_finite_positive({ap->dark_eps})) return fail(MI355PT_E_INVALID, "adaptive: dark_eps must be finite and > 0");
    if (ap->min_spp < 2u || (ap->min_spp & (ap->min_spp - 1u)) != 0u) return fail(MI355PT_E_INVALID, "adaptive: min_spp must be a power of two >= 2");
    return MI355PT_OK;
}
static int adaptive_check_scratch(uint32_t width, uint32_t height, const void* d_scratch, size_t scratch_bytes) {
    if (width == 0 || height == 0 || adaptive_tile_count(width, height) == 0u) return fail(MI355PT_E_INVALID, "adaptive: zero width or height, or a frame of 2^31 tiles or more");
    const Scratch sv = scratch_verdict(d_scratch, scratch_bytes, adaptive_scratch_bytes(width, height), 4);
    if (sv == Scratch::MISSING || sv == Scratch::TOO_SMALL) return fail(MI355PT_E_INVALID, "adaptive: scratch missing or smaller than mi355pt_adaptive_scratch_bytes");
    if (sv == Scratch::MISALIGNED) return fail(MI355PT_E_INVALID, "adaptive: scratch is not 4-byte aligned");
    return MI355PT_OK;
}

// every check of the two drivers that does not concern the device buffers
static int adaptive_check_render(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const mi355pt_adaptive_params* ap) {
    int rc = check_tiles_args(s, cam, p);
    if (rc) return rc;
    if ((rc = adaptive_check_params(ap))) return rc;
    if ((p->spp & (p->spp - 1u)) != 0u || p->spp < ap->min_spp) return fail(MI355PT_E_INVALID, "adaptive: spp (the maximum) must be a power of two >= min_spp");
    return MI355PT_OK;
}

extern "C" {

size_t mi355pt_adaptive_scratch_bytes(uint32_t width, uint32_t height) { return adaptive_scratch_bytes(width, height); }

int mi355pt_adaptive_step_device(const float* d_film, float* d_half, uint32_t width, uint32_t height, uint32_t* d_tile_spp, float* d_tile_err,
                                 const mi355pt_adaptive_params* ap, uint32_t level_spp, uint32_t max_spp, void* d_scratch, size_t scratch_bytes,
                                 uint32_t* d_list, uint32_t* d_count, void* hip_stream) {
    int rc = adaptive_check_params(ap);
    if (rc) return rc;
    if (!d_film || !d_half || !d_tile_spp || !d_tile_err || !d_list || !d_count) return fail(MI355PT_E_INVALID, "adaptive: null buffer");
    if (level_spp == 0u || (level_spp & 1u) != 0u) return fail(MI355PT_E_INVALID, "adaptive: level_spp must be even and > 0");
    if (max_spp < level_spp) return fail(MI355PT_E_INVALID, "adaptive: max_spp is below level_spp");
    if ((rc = adaptive_check_scratch(width, height, d_scratch, scratch_bytes))) return rc;
    HIP_TRY(launch_adaptive_step(d_film, d_half, width, height, d_tile_spp, d_tile_err, ap->threshold, ap->dark_eps, level_spp, max_spp, d_scratch, d_list,
                                 d_count, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_film_normalize_tiles_device(const float* d_film, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_mean, void* hip_stream) {
    if (!d_film || !d_tile_spp || !d_mean) return fail(MI355PT_E_INVALID, "normalize: null buffer");
    if (width == 0 || height == 0 || adaptive_tile_count(width, height) == 0u) return fail(MI355PT_E_INVALID, "normalize: zero width or height, or a frame of 2^31 tiles or more");
    HIP_TRY(launch_normalize_tiles(d_film, d_tile_spp, width, height, d_mean, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_render_adaptive_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const mi355pt_adaptive_params* ap,
                                   float* d_film, float* d_half, uint32_t* d_tile_spp, float* d_tile_err, uint32_t* d_list, void* d_scratch,
                                   size_t scratch_bytes, void* hip_stream, mi355pt_adaptive_result* result) {
    int rc = adaptive_check_render(s, cam, p, ap);
    if (rc) return rc;
    if (!d_film || !d_half || !d_tile_spp || !d_tile_err || !d_list) return fail(MI355PT_E_INVALID, "adaptive: null buffer");
    if ((rc = adaptive_check_scratch(cam->width, cam->height, d_scratch, scratch_bytes))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const uint32_t W = cam->width, H = cam->height, n_tiles = adaptive_tile_count(W, H), tiles_x = (W + 7u) / 8u;
    const uint32_t min_spp = ap->min_spp, max_spp = p->spp;
    const size_t film_bytes = (size_t)W * H * 3 * sizeof(float);
    uint32_t* d_count = (uint32_t*)((char*)d_scratch + adaptive_scratch_bytes(W, H) - 16u);     // the scratch's last 16 bytes
    const PathOut no_log{nullptr, nullptr, nullptr, 0u, 0u};
    // 1 - 4: every tile at min_spp, H = [0, min / 2), F = [0, min)
    HIP_TRY(hipMemsetAsync(d_film, 0, film_bytes, stream));
    HIP_TRY(hipMemsetAsync(d_half, 0, film_bytes, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_tile_spp, (int)min_spp, n_tiles, stream));
    if ((rc = render_accum_range(s, cam, p, 0u, min_spp / 2u, d_half, hip_stream, nullptr, no_log))) return rc;
    HIP_TRY(hipMemcpyAsync(d_film, d_half, film_bytes, hipMemcpyDeviceToDevice, stream));
    if ((rc = render_accum_range(s, cam, p, min_spp / 2u, min_spp, d_film, hip_stream, nullptr, no_log))) return rc;
    // 5: step, count, the listed tiles' next samples
    uint32_t passes = 0;
    for (uint32_t level = min_spp; level <= max_spp; level *= 2u) {
        HIP_TRY(launch_adaptive_step(d_film, d_half, W, H, d_tile_spp, d_tile_err, ap->threshold, ap->dark_eps, level, max_spp, d_scratch, d_list, d_count, stream));
        ++passes;
        uint32_t count = 0;
        HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (count == 0u) break;                              // (at level == max_spp always: the step activates nothing there)
        if (count > n_tiles) return fail(MI355PT_E_DEVICE, "adaptive: the step returned more tiles than the frame has");
        if ((rc = launch_ranges(s, cam, p, level, 2u * level, d_film, stream, nullptr, d_list, count))) return rc;
    }
    if (result) {
        std::vector<uint32_t> spp(n_tiles);
        HIP_TRY(hipMemcpyAsync(spp.data(), d_tile_spp, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        result->passes = passes; result->tiles_at_max = 0; result->total_samples = 0;
        for (uint32_t t = 0; t < n_tiles; ++t) {
            const uint32_t tw = std::min(8u, W - (t % tiles_x) * 8u), th = std::min(8u, H - (t / tiles_x) * 8u);
            result->total_samples += (uint64_t)spp[t] * tw * th;
            result->tiles_at_max += spp[t] == max_spp ? 1u : 0u;
        }
    }
    return MI355PT_OK;
}

int mi355pt_render_adaptive(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const mi355pt_adaptive_params* ap, float* out_rgb,
                            uint32_t* out_tile_spp, mi355pt_adaptive_result* result) {
    int rc = adaptive_check_render(s, cam, p, ap);
    if (rc) return rc;
    if (!out_rgb) return fail(MI355PT_E_INVALID, "null output");
    const uint32_t W = cam->width, H = cam->height, n_tiles = adaptive_tile_count(W, H);
    const size_t n = (size_t)W * H * 3, scratch_bytes = adaptive_scratch_bytes(W, H);
    DevBuf<float> d_film, d_half, d_err;
    DevBuf<uint32_t> d_spp, d_list;
    DevBuf<unsigned char> d_scratch;
    HIP_TRY(d_film.alloc(n)); HIP_TRY(d_half.alloc(n)); HIP_TRY(d_err.alloc(n_tiles)); HIP_TRY(d_spp.alloc(n_tiles)); HIP_TRY(d_list.alloc(n_tiles));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    if ((rc = mi355pt_render_adaptive_device(s, cam, p, ap, d_film.p, d_half.p, d_spp.p, d_err.p, d_list.p, d_scratch.p, scratch_bytes, nullptr, result))) return rc;
    // the half film has done its work: it takes the means, and the film the resolved frame
    if ((rc = mi355pt_film_normalize_tiles_device(d_film.p, d_spp.p, W, H, d_half.p, nullptr))) return rc;
    if ((rc = mi355pt_film_resolve_device(d_half.p, W * H, 1u, d_film.p, nullptr))) return rc;
    HIP_TRY(d_film.download(out_rgb, n));
    HIP_TRY(d_spp.download(out_tile_spp, n_tiles));
    return MI355PT_OK;
}

}  // extern "C"
