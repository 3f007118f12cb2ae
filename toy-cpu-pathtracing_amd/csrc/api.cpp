// The core of libmi355pt.so's extern "C" boundary (include/mi355pt.h): the error string and the version, the argument checks every render
// entry point shares, the launch context and the launches over it, and the plain, tile-list and AOV render and resolve entry points.  Every
// other public header has a file of its own: api_scene.cpp (the scene description and build), api_multi.cpp (several GPUs), api_denoise.cpp,
// api_adaptive.cpp, api_gbuffer.cpp, api_temporal.cpp, api_upsample.cpp, api_display.cpp, api_robust.cpp, api_debug.cpp; what they share is
// api_internal.hpp.  Host C++ only; the compute lives in pt_kernels.hip, the launch shape in launch_plan.hpp.
#include <cstring>

#include "api_internal.hpp"

using namespace pt;

static thread_local std::string g_err;
bool pt::g_debug_unlocked = false;
int pt::fail(int code, const std::string& msg) { g_err = msg; return code; }

static const uint32_t CIE_CMF_BITS[470 * 4] = {
#include "cie_cmf.inc"
};
void pt::cie_cmf4(float out[470 * 4]) { std::memcpy(out, CIE_CMF_BITS, sizeof(CIE_CMF_BITS)); }

int pt::get_launch_ctx(const mi355pt_scene* sc, uint32_t seed, LaunchCtx** out, int* slot) {
    // (check_args has made sure that the current device is the one the scene was built on)
    if (sc->ctx && sc->ctx->device != sc->impl.device) {
        // the scene was rebuilt on another device since its last render (mi355pt_scene_build after hipSetDevice, or build_multi with a
        // different first device): the hash table, counters, stats and partial film of the old context live in the OLD device's memory
        delete sc->ctx; sc->ctx = nullptr;
    }
    if (!sc->ctx) {
        LaunchCtx* lc = new LaunchCtx();
        lc->device = sc->impl.device;
        HIP_TRY(hipMalloc((void**)&lc->d_hash, sizeof(uint64_t) * HASH_TABLE_DIMS));
        HIP_TRY(hipMalloc((void**)&lc->d_counters, sizeof(unsigned) * CTX_RING));
        HIP_TRY(hipMalloc((void**)&lc->d_stats, sizeof(DevStats) * CTX_RING));
        sc->ctx = lc;
    }
    LaunchCtx* lc = sc->ctx;
    if (!lc->hash_valid || lc->hash_seed != seed) {
        std::vector<uint64_t> tab(HASH_TABLE_DIMS);
        for (int i = 0; i < HASH_TABLE_DIMS; ++i) tab[i] = host_murmur_dim_seed((uint32_t)i, seed);
        // a seed change is rare (the CLI renders one seed): synchronous copy, ordered after any in-flight launch
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(lc->d_hash, tab.data(), sizeof(uint64_t) * HASH_TABLE_DIMS, hipMemcpyHostToDevice));
        lc->hash_seed = seed; lc->hash_valid = true;
    }
    *slot = lc->next; lc->next = (lc->next + 1) % CTX_RING;
    *out = lc;
    return MI355PT_OK;
}

namespace {

// a buffer of the launch context that must hold `need` bytes: an earlier launch on `stream` may still be using the old one
template <typename T>
int grow_device_buffer(T** ptr, size_t* have, size_t need, hipStream_t stream) {
    if (need <= *have) return MI355PT_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipFree(*ptr); *ptr = nullptr; *have = 0;
    HIP_TRY(hipMalloc((void**)ptr, need));
    *have = need;
    return MI355PT_OK;
}

void copy_stats(const DevStats& h, mi355pt_stats* stats) {
    stats->samples = h.samples; stats->closest_rays = h.closest_rays; stats->shadow_rays = h.shadow_rays;
    stats->nodes_closest = h.nodes_closest; stats->tris_closest = h.tris_closest; stats->nodes_shadow = h.nodes_shadow;
    stats->tris_shadow = h.tris_shadow; stats->closest_hits = h.closest_hits; stats->bounces = h.bounces;
    stats->spectrum_evals = h.spectrum_evals; stats->textured_lookups = h.textured_lookups;
    for (int i = 0; i < 10; ++i) stats->phase_cycles[i] = h.phase_cycles[i];
    for (int i = 0; i < 8; ++i) stats->wave_steps[i] = h.wave_steps[i];
    for (int i = 0; i < 16; ++i) stats->busy_hist[i] = h.busy_hist[i >> 3][i & 7];
    for (int i = 0; i < 12; ++i) stats->divergence[i] = h.divergence[i];
}

}  // namespace

int pt::timed_launch(LaunchCtx* lc, int slot, hipStream_t stream, mi355pt_stats* stats, bool counts,
                     const std::function<int(unsigned* d_counter, DevStats* d_stats)>& launch) {
    unsigned* d_counter = lc->d_counters + slot;
    DevStats* d_stats = lc->d_stats + slot;
    HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(unsigned), stream));
    if (stats && counts) HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), stream));
    Event e0, e1;
    if (stats) { HIP_TRY(e0.create()); HIP_TRY(e1.create()); HIP_TRY(e0.record(stream)); }
    if (int rc = launch(d_counter, d_stats)) return rc;
    if (stats) {
        HIP_TRY(e1.record(stream));
        HIP_TRY(e1.synchronize());
        float ms = 0.0f;
        HIP_TRY(e1.elapsed_ms(e0, &ms));
        std::memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms; stats->launches = 1;
        if (counts) {
            DevStats h;
            HIP_TRY(hipMemcpy(&h, d_stats, sizeof(h), hipMemcpyDeviceToHost));
            copy_stats(h, stats);
        }
    }
    return MI355PT_OK;   // stats == NULL: fully asynchronous on `stream`
}

int pt::check_args(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, bool aov) {
    if (!s || !cam || !p) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (cam->width == 0 || cam->height == 0 || p->spp == 0) return fail(MI355PT_E_INVALID, "empty image or spp == 0");
    if ((!aov && p->strategy > 2) || p->sampler > 1) return fail(MI355PT_E_INVALID, "bad strategy/sampler");
    // the path records of the kernels' queues hold the depth in 10 bits and the sampler dimension in 15: a path draws 3 dimensions at the
    // camera and at most 8 per bounce, so 3 + 8 * 1000 = 8003 < 2^15 (tests/test_oracle.py checks the deepest dimension the oracle's paths reach)
    if (!aov && p->max_depth > 1000u) return fail(MI355PT_E_INVALID, "max_depth > 1000 (the path records of the kernel's queues hold the depth in 10 bits and the sampler dimension in 15)");
    if (!(p->rr_gate_slack >= 0.0f && p->rr_gate_slack < 1.0f)) return fail(MI355PT_E_INVALID, "rr_gate_slack must be in [0, 1)");
    if (p->rr_gate_slack != 0.0f && !g_debug_unlocked)
        return fail(MI355PT_E_INVALID, "mi355pt_params.rr_gate_slack must be 0 (a diagnostic: mi355pt_debug_unlock(1) in mi355pt_debug.h enables it)");
    if (p->shard_count && p->shard_index >= p->shard_count) return fail(MI355PT_E_INVALID, "bad shard");
    // mi355pt_scene_build bakes the world -> render translation (render space = world - camera position, camera.rs:84-86) into every
    // device record and uploads to the device that was current then: a render call must name the same camera position and device
    if (std::memcmp(cam->position, s->impl.build_cam_pos, sizeof(float) * 3) != 0)
        return fail(MI355PT_E_INVALID, "camera position differs from the one given to mi355pt_scene_build: rebuild the scene");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->impl.device)
        return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    return MI355PT_OK;
}

// one launch of a sample range (arguments checked): plan -> context / buffers -> memsets -> launch -> stats.  d_list != nullptr: the tile-list
// kernels over d_list[0 .. n_list) (device memory, n_list > 0; no AOV kind, no instrumentation, no sample log).
// Their shape is planned with the resident waves of the PLAIN kernel of the same mode: chunks and block size — the frame's bits — then equal
// plan_launch's for a list of all tiles, whatever occupancy the tile-list instantiation has (a grid that does not fit waits its turn: the
// work items are independent).
static int launch_range(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, float* d_accum,
                        hipStream_t stream, mi355pt_stats* stats, const PathOut& pout, int aov_kind, uint32_t illuminant_lut, const uint32_t* d_list,
                        uint32_t n_list) {
    const bool aov = aov_kind >= 0;
    if (!d_list && shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) == 0) return MI355PT_OK;
    int rc;
    LaunchCtx* lc; int slot;
    if ((rc = get_launch_ctx(s, p->seed, &lc, &slot))) return rc;
    if (lc->device != s->impl.device) return fail(MI355PT_E_DEVICE, "launch context and scene live on different devices");
    const bool want_stats = stats && p->collect_stats;
    // the persistent grid of the exact kernel of this scene's feature set on this scene's device: asked once, then cached
    int& waves = aov ? lc->aov_waves[aov_kind] : lc->waves[want_stats ? 1 : 0][p->sampler & 1u][p->strategy < 3u ? p->strategy : 0u];
    if (!waves) waves = aov ? query_resident_waves_aov((uint32_t)aov_kind, s->impl.features)
                            : query_resident_waves(select_kernel(false, want_stats, s->impl.features, p->sampler, p->strategy));
    const DevCamera dc = make_camera(cam);
    LaunchPlan plan = d_list ? plan_launch_tiles(cam, p, s_begin, s_end, waves, n_list) : plan_launch(cam, p, s_begin, s_end, waves, aov);
    DevParams& dp = plan.params;
    if (d_list) set_tile_list(dp, d_list);
    dp.stats_mode = p->collect_stats;
    // (the AOV kernel counts its samples, primary rays and hits in every launch that is given a stats block)
    // (a production launch that is given a stats block after mi355pt_debug_unlock(1) counts the rays it did not trace — path_end_plan.hpp — into
    // wave_steps[7]; every other production launch passes its kernel no stats pointer)
    const bool count_ends = stats && !want_stats && !aov && g_debug_unlocked;
    return timed_launch(lc, slot, stream, stats, want_stats || aov || count_ends, [&](unsigned* d_counter, DevStats* d_stats) {
        if ((rc = grow_device_buffer(&lc->d_partial, &lc->partial_bytes, plan.partial_floats * sizeof(float), stream))) return rc;
        // (one stream at a time per scene, like d_partial: the queues are empty between launches, so consecutive launches share them)
        // (sized by what the selected kernel's queues use per wave; the buffer only grows: a context that launches several kernels holds the largest)
        const KernelKey key = select_kernel(d_list != nullptr, want_stats, s->impl.features, p->sampler, p->strategy);
        if ((rc = grow_device_buffer(&lc->d_defer, &lc->defer_bytes, aov ? (size_t)0 : query_defer_bytes_per_wave(key) * (size_t)plan.grid, stream))) return rc;
        if (aov) HIP_TRY(launch_aov((uint32_t)aov_kind, s->impl.dev, dc, dp, illuminant_lut, lc->d_hash, d_accum, d_counter, stats ? d_stats : nullptr,
                                    s->impl.features, plan.grid, stream));
        else {
            DevScene dev = s->impl.dev;
            dev.cam_lists = use_camera_lists(key, dp.block_log2, camera_lists_enabled()) ? 1u : 0u;
            dev.queue_stage = use_queue_staging(key, queue_staging_enabled()) ? 1u : 0u;
            dev.light_queue = use_light_queue(key, light_queue_enabled()) ? 1u : 0u;
            dev.early_path_end = use_early_path_end(key, early_path_end_enabled()) ? 1u : 0u;
            HIP_TRY(launch_pt(key, dev, dc, dp, plan.n_tiles,
                              lc->d_hash, d_accum, lc->d_partial, d_counter, (want_stats && !d_list) || count_ends ? d_stats : nullptr, plan.grid, stream, pout, lc->d_defer));
        }
        return (int)MI355PT_OK;
    });
}

int pt::launch_ranges(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, float* d_accum,
                      hipStream_t stream, mi355pt_stats* stats, const uint32_t* d_list, uint32_t n_list, const PathOut& pout, int aov_kind,
                      uint32_t illuminant_lut) {
    return for_each_launch_range(p->sampler, stats != nullptr, s_begin, s_end, [&](uint32_t b, uint32_t e) {
        return launch_range(s, cam, p, b, e, d_accum, stream, stats, pout, aov_kind, illuminant_lut, d_list, n_list);
    });
}

int pt::render_accum_range(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end,
                           float* d_accum, void* hip_stream, mi355pt_stats* stats, const PathOut& pout, int aov_kind, uint32_t illuminant_lut) {
    const bool aov = aov_kind >= 0;
    int rc = check_args(s, cam, p, aov);
    if (rc) return rc;
    if (!d_accum || s_end > p->spp || s_begin >= s_end) return fail(MI355PT_E_INVALID, "bad sample range or null accumulator");
    if (aov) {
        if (aov_kind > MI355PT_AOV_SHADING_NORMAL) return fail(MI355PT_E_INVALID, "unknown AOV kind");
        if (p->collect_stats) return fail(MI355PT_E_INVALID, "the AOV renderers have no instrumented kernel: collect_stats must be 0");
        if (aov_kind == MI355PT_AOV_ALBEDO && illuminant_lut >= s->impl.luts.size())
            return fail(MI355PT_E_INVALID, "illuminant_lut is not a LUT470 id of this scene (presets::cie_illum_d6500())");
    }
    return launch_ranges(s, cam, p, s_begin, s_end, d_accum, (hipStream_t)hip_stream, stats, nullptr, 0u, pout, aov_kind, illuminant_lut);
}

int pt::check_tiles_args(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p) {
    int rc = check_args(s, cam, p);
    if (rc) return rc;
    if (p->shard_count > 1u) return fail(MI355PT_E_INVALID, "tile lists name tiles of the whole frame: shard_count must be 0 or 1");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "there is no instrumented tile-list kernel: collect_stats must be 0");
    if (adaptive_tile_count(cam->width, cam->height) == 0u) return fail(MI355PT_E_INVALID, "the frame has 2^31 tiles or more");
    return MI355PT_OK;
}

extern "C" {

const char* mi355pt_last_error(void) { return g_err.c_str(); }
#ifndef MI355PT_BUILD_ID
#define MI355PT_BUILD_ID "dev"
#endif
const char* mi355pt_version(void) { return "mi355pt 0.2.0 (gfx950) build " MI355PT_BUILD_ID; }

int mi355pt_render_accum_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end,
                                float* d_accum, void* hip_stream, mi355pt_stats* stats) {
    return render_accum_range(s, cam, p, s_begin, s_end, d_accum, hip_stream, stats, PathOut{nullptr, nullptr, nullptr, 0u, 0u});
}

int mi355pt_render_accum_tiles_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const uint32_t* tiles, uint32_t n_tiles,
                                      uint32_t s_begin, uint32_t s_end, float* d_accum, void* hip_stream, mi355pt_stats* stats) {
    int rc = check_tiles_args(s, cam, p);
    if (rc) return rc;
    if (!d_accum || s_end > p->spp || s_begin >= s_end) return fail(MI355PT_E_INVALID, "bad sample range or null accumulator");
    if (n_tiles && !tiles) return fail(MI355PT_E_INVALID, "null tile list");
    const uint32_t total = adaptive_tile_count(cam->width, cam->height);
    for (uint32_t k = 0; k < n_tiles; ++k) {
        if (tiles[k] >= total) return fail(MI355PT_E_INVALID, "tile index at or beyond the frame's tile count");
        if (k && tiles[k] <= tiles[k - 1]) return fail(MI355PT_E_INVALID, "the tile list must be strictly ascending");
    }
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n_tiles == 0) return MI355PT_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    LaunchCtx* lc; int slot;
    if ((rc = get_launch_ctx(s, p->seed, &lc, &slot))) return rc;
    if ((rc = grow_device_buffer(&lc->d_tiles, &lc->tiles_bytes, (size_t)n_tiles * sizeof(uint32_t), stream))) return rc;
    // (ordered on the stream after an earlier launch that may still read the buffer; the caller's array is free again when this returns)
    HIP_TRY(hipMemcpyAsync(lc->d_tiles, tiles, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return launch_ranges(s, cam, p, s_begin, s_end, d_accum, stream, stats, lc->d_tiles, n_tiles);
}

int mi355pt_film_resolve_device(const float* d_accum, uint32_t n_pixels, uint32_t spp, float* d_out, void* hip_stream) {
    if (!d_accum || !d_out || spp == 0) return fail(MI355PT_E_INVALID, "bad resolve arguments");
    HIP_TRY(launch_resolve(d_accum, n_pixels * 3, spp, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_render_aov_accum_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, int kind, uint32_t illuminant_lut,
                                    uint32_t s_begin, uint32_t s_end, float* d_accum, void* hip_stream, mi355pt_stats* stats) {
    if (kind < MI355PT_AOV_NORMAL || kind > MI355PT_AOV_SHADING_NORMAL) return fail(MI355PT_E_INVALID, "unknown AOV kind");
    return render_accum_range(s, cam, p, s_begin, s_end, d_accum, hip_stream, stats, PathOut{nullptr, nullptr, nullptr, 0u, 0u}, kind, illuminant_lut);
}
int mi355pt_aov_resolve_device(int kind, const float* d_accum, uint32_t n_pixels, uint32_t spp, float* d_out, void* hip_stream) {
    if (kind < MI355PT_AOV_NORMAL || kind > MI355PT_AOV_SHADING_NORMAL) return fail(MI355PT_E_INVALID, "unknown AOV kind");
    if (!d_accum || !d_out || spp == 0) return fail(MI355PT_E_INVALID, "bad resolve arguments");
    HIP_TRY(launch_aov_resolve((uint32_t)kind, d_accum, n_pixels * 3, spp, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}
// mi355pt_render (aov_kind < 0) and mi355pt_render_aov: alloc, zero, accumulate, resolve, copy out
static int render_to_host(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, int aov_kind, uint32_t illuminant_lut,
                          float* out_rgb, mi355pt_stats* stats) {
    const bool aov = aov_kind >= 0;
    int rc = check_args(s, cam, p, aov);
    if (rc) return rc;
    if (!out_rgb) return fail(MI355PT_E_INVALID, "null output");
    size_t n = (size_t)cam->width * cam->height * 3;
    DevBuf<float> d_acc, d_out;
    HIP_TRY(d_acc.alloc(n));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(hipMemset(d_acc.p, 0, n * sizeof(float)));
    if ((rc = aov ? mi355pt_render_aov_accum_device(s, cam, p, aov_kind, illuminant_lut, 0, p->spp, d_acc.p, nullptr, stats)
                  : mi355pt_render_accum_device(s, cam, p, 0, p->spp, d_acc.p, nullptr, stats))) return rc;
    if ((rc = aov ? mi355pt_aov_resolve_device(aov_kind, d_acc.p, cam->width * cam->height, p->spp, d_out.p, nullptr)
                  : mi355pt_film_resolve_device(d_acc.p, cam->width * cam->height, p->spp, d_out.p, nullptr))) return rc;
    HIP_TRY(d_out.download(out_rgb, n));
    return MI355PT_OK;
}
int mi355pt_render_aov(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, int kind, uint32_t illuminant_lut, float* out_rgb,
                       mi355pt_stats* stats) {
    if (kind < MI355PT_AOV_NORMAL || kind > MI355PT_AOV_SHADING_NORMAL) return fail(MI355PT_E_INVALID, "unknown AOV kind");
    return render_to_host(s, cam, p, kind, illuminant_lut, out_rgb, stats);
}
int mi355pt_render(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, float* out_rgb, mi355pt_stats* stats) {
    return render_to_host(s, cam, p, -1, 0u, out_rgb, stats);
}

}  // extern "C"
