// The mi355pt_gbuffer.h surface of libmi355pt.so: the argument checks, the launch's shape and the three entry points of the G-buffer pass.
// Host C++ only, like api.cpp, whose launch context and timed launch it uses; the kernels are in pt_kernels_gbuffer.hip.
#include "api_internal.hpp"

using namespace pt;

// every check of the two G-buffer render entry points; the refusals the header lists come first and look at host memory only
static int gbuffer_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut, uint32_t s_begin,
                         uint32_t s_end, const mi355pt_gbuffer_films* films) {
    if (!films) return fail(MI355PT_E_INVALID, "gbuffer: null films struct");
    const float* f[4] = {films->albedo, films->shading_normal, films->position, films->hit};
    if (!f[0] && !f[1] && !f[2] && !f[3]) return fail(MI355PT_E_INVALID, "gbuffer: no film requested (all four pointers are NULL)");
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (f[i] && f[i] == f[j]) return fail(MI355PT_E_INVALID, "gbuffer: two film pointers are equal");
    if (!s || !cam || !p) return fail(MI355PT_E_INVALID, "null argument");
    if (s_end > p->spp || s_begin > s_end) return fail(MI355PT_E_INVALID, "gbuffer: bad sample range");
    if (cam->width == 0 || cam->height == 0) return fail(MI355PT_E_INVALID, "gbuffer: zero-sized frame");
    if (films->albedo && illuminant_lut >= s->impl.luts.size())
        return fail(MI355PT_E_INVALID, "gbuffer: illuminant_lut is not a LUT470 id of this scene (presets::cie_illum_d6500())");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "the G-buffer pass has no instrumented kernel: collect_stats must be 0");
    return check_args(s, cam, p, true);
}

// The G-buffer launch's shape: the AOV plan (never a split sample range) with the work item pinned to a whole 8x8 tile, whatever the sample
// count — one pixel per lane, so that the kernel keeps a pixel's sums in the owning lane's registers (pt_kernels_gbuffer.hip)
static LaunchPlan plan_gbuffer(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, int waves) {
    LaunchPlan plan = plan_launch(cam, p, s_begin, s_end, waves, true);
    DevParams& dp = plan.params;
    dp.block_log2 = 3u; dp.sample_prefix_digits = 0u;
    dp.n_work = plan.n_tiles * dp.chunks;                      // (chunks == 1)
    plan.grid = (int)std::min<uint32_t>(dp.n_work, (uint32_t)waves);
    return plan;
}

// one launch of a sample range (arguments checked), after api.cpp's launch_range; the kernel counts in every launch that is given a stats block
static int launch_gbuffer_range(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut, uint32_t s_begin,
                                uint32_t s_end, const mi355pt_gbuffer_films* films, hipStream_t stream, mi355pt_stats* stats) {
    if (s_begin == s_end || shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) == 0) return MI355PT_OK;
    int rc;
    LaunchCtx* lc; int slot;
    if ((rc = get_launch_ctx(s, p->seed, &lc, &slot))) return rc;
    if (lc->device != s->impl.device) return fail(MI355PT_E_DEVICE, "launch context and scene live on different devices");
    if (!lc->gbuffer_waves) lc->gbuffer_waves = query_resident_waves_gbuffer(s->impl.features);
    const DevCamera dc = make_camera(cam);
    LaunchPlan plan = plan_gbuffer(cam, p, s_begin, s_end, lc->gbuffer_waves);
    plan.params.stats_mode = 0u;
    const GbufferFilms gf{films->albedo, films->shading_normal, films->position, films->hit};
    return timed_launch(lc, slot, stream, stats, true, [&](unsigned* d_counter, DevStats* d_stats) {
        HIP_TRY(launch_gbuffer(s->impl.dev, dc, plan.params, illuminant_lut, lc->d_hash, gf, d_counter, stats ? d_stats : nullptr, s->impl.features, plan.grid,
                               stream));
        return (int)MI355PT_OK;
    });
}

extern "C" {

int mi355pt_render_gbuffer_accum_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut,
                                        uint32_t s_begin, uint32_t s_end, const mi355pt_gbuffer_films* films, void* hip_stream, mi355pt_stats* stats) {
    int rc = gbuffer_check(s, cam, p, illuminant_lut, s_begin, s_end, films);
    if (rc) return rc;
    return for_each_launch_range(p->sampler, stats != nullptr, s_begin, s_end, [&](uint32_t b, uint32_t e) {
        return launch_gbuffer_range(s, cam, p, illuminant_lut, b, e, films, (hipStream_t)hip_stream, stats);
    });
}

int mi355pt_gbuffer_normalize_device(const float* d_film, const float* d_hit, uint32_t n_pixels, float* d_out, void* hip_stream) {
    if (!d_film || !d_hit || !d_out) return fail(MI355PT_E_INVALID, "gbuffer normalize: null buffer");
    if (d_out == d_film || d_out == d_hit) return fail(MI355PT_E_INVALID, "gbuffer normalize: the output must not be one of the inputs");
    HIP_TRY(launch_gbuffer_normalize(d_film, d_hit, n_pixels, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_render_gbuffer(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut,
                           const mi355pt_gbuffer_films* out, mi355pt_stats* stats) {
    int rc = gbuffer_check(s, cam, p, illuminant_lut, 0u, p ? p->spp : 0u, out);
    if (rc) return rc;
    const size_t n = (size_t)cam->width * cam->height * 3;
    float* const host[4] = {out->albedo, out->shading_normal, out->position, out->hit};
    DevBuf<float> d_acc[4], d_res;
    HIP_TRY(d_res.alloc(n));
    for (int i = 0; i < 4; ++i)
        if (host[i]) { HIP_TRY(d_acc[i].alloc(n)); HIP_TRY(hipMemset(d_acc[i].p, 0, n * sizeof(float))); }
    const mi355pt_gbuffer_films dev{d_acc[0].p, d_acc[1].p, d_acc[2].p, d_acc[3].p};
    if ((rc = mi355pt_render_gbuffer_accum_device(s, cam, p, illuminant_lut, 0u, p->spp, &dev, nullptr, stats))) return rc;
    for (int i = 0; i < 4; ++i) {
        if (!host[i]) continue;
        // albedo: Sensor::to_rgb with NoneToneMap; the other films: sum / spp, raw (the resolve of the shading-normal kind)
        if ((rc = mi355pt_aov_resolve_device(i == 0 ? MI355PT_AOV_ALBEDO : MI355PT_AOV_SHADING_NORMAL, d_acc[i].p, cam->width * cam->height, p->spp,
                                             d_res.p, nullptr))) return rc;
        HIP_TRY(d_res.download(host[i], n));
    }
    return MI355PT_OK;
}

}  // extern "C"
