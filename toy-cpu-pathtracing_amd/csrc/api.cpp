// extern "C" boundary of libmi355pt.so (include/mi355pt.h, mi355pt_denoise.h, mi355pt_denoise_var.h, mi355pt_adaptive.h, mi355pt_gbuffer.h; api_debug.cpp holds mi355pt_debug.h's).  Host C++ only;
// the compute lives in pt_kernels.hip, the launch shape in launch_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt.h"
#include "api_internal.hpp"

using namespace pt;

static thread_local std::string g_err;
bool pt::g_debug_unlocked = false;
int pt::fail(int code, const std::string& msg) { g_err = msg; return code; }

static const uint32_t CIE_CMF_BITS[470 * 4] = {
#include "cie_cmf.inc"
};
void pt::cie_cmf4(float out[470 * 4]) { std::memcpy(out, CIE_CMF_BITS, sizeof(CIE_CMF_BITS)); }

namespace {

// returns the scene's launch context with the hash table valid for `seed`; `slot` receives a fresh ring slot
int get_launch_ctx(const mi355pt_scene* sc, uint32_t seed, LaunchCtx** out, int* slot) {
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

static void free_parts(std::vector<MultiPart>& parts) {
    for (size_t i = 0; i < parts.size(); ++i) {
        MultiPart& m = parts[i];
        (void)hipSetDevice(m.device);
        if (m.stream) (void)hipStreamDestroy(m.stream);
        if (m.done) (void)hipEventDestroy(m.done);
        (void)hipFree(m.d_film); (void)hipFree(m.d_pack); (void)hipFree(m.d_stage); (void)hipFree(m.d_out);
        if (i > 0) delete m.scene;
    }
    parts.clear();
}
mi355pt_scene::~mi355pt_scene() {
    int cur = 0;
    const bool have = !parts.empty() && hipGetDevice(&cur) == hipSuccess;
    free_parts(parts);
    if (have) (void)hipSetDevice(cur);
    delete ctx;
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
    unsigned* d_counter = lc->d_counters + slot;
    DevStats* d_stats = lc->d_stats + slot;
    HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(unsigned), stream));
    dp.stats_mode = p->collect_stats;
    if (want_stats || (aov && stats)) HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (stats) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, stream)); }
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
        HIP_TRY(launch_pt(key, dev, dc, dp, plan.n_tiles,
                          lc->d_hash, d_accum, lc->d_partial, d_counter, d_list ? nullptr : d_stats, plan.grid, stream, pout, lc->d_defer));
    }
    if (stats) {
        HIP_TRY(hipEventRecord(e1, stream));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        std::memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms; stats->launches = 1;
        if (want_stats || aov) {   // the AOV kernel counts its samples, primary rays and hits in every launch that is given a stats block
            DevStats h;
            HIP_TRY(hipMemcpy(&h, d_stats, sizeof(h), hipMemcpyDeviceToHost));
            copy_stats(h, stats);
        }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return MI355PT_OK;   // stats == NULL: fully asynchronous on `stream`
}

// the launches of [s_begin, s_end) into d_accum, arguments checked; with d_list, of the tiles d_list[0 .. n_list) (device memory)
static int launch_ranges(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, float* d_accum,
                         hipStream_t stream, mi355pt_stats* stats, const uint32_t* d_list, uint32_t n_list,
                         const PathOut& pout = PathOut{nullptr, nullptr, nullptr, 0u, 0u}, int aov_kind = -1, uint32_t illuminant_lut = 0) {
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

// what the tile-list entry and the adaptive driver ask of (scene, camera, params) beyond check_args
static int check_tiles_args(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p) {
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

int mi355pt_scene_create(mi355pt_scene** out) {
    if (!out) return fail(MI355PT_E_INVALID, "null out");
    *out = new (std::nothrow) mi355pt_scene();
    return *out ? MI355PT_OK : fail(MI355PT_E_INVALID, "allocation failed");
}
void mi355pt_scene_destroy(mi355pt_scene* s) { delete s; }

int mi355pt_scene_set_rgb2spec(mi355pt_scene* s, const float* table, size_t n) {
    if (!s || !table || n != (size_t)(64 + 3 * 64 * 64 * 64 * 3)) return fail(MI355PT_E_INVALID, "rgb2spec table must have 64 + 3*64^3*3 floats");
    s->impl.table.assign(table, table + n);
    return MI355PT_OK;
}
int mi355pt_scene_add_lut470(mi355pt_scene* s, const float* v, uint32_t* id) {
    if (!s || !v || !id) return fail(MI355PT_E_INVALID, "null argument");
    s->impl.luts.emplace_back(v, v + 470);
    *id = (uint32_t)s->impl.luts.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_tex_rgb8(mi355pt_scene* s, const uint8_t* rgb, uint32_t w, uint32_t h, uint32_t* id) {
    if (!s || !rgb || !id || w == 0 || h == 0) return fail(MI355PT_E_INVALID, "bad texture");
    SceneImpl::Tex t; t.w = w; t.h = h; t.rgb.assign(rgb, rgb + (size_t)w * h * 3);
    s->impl.textures.push_back(std::move(t));
    *id = (uint32_t)s->impl.textures.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_mesh(mi355pt_scene* s, const float* pos, const float* nrm, const float* uv, const float* tri_tangent, const uint32_t* idx,
                           uint32_t nv, uint32_t nt, uint32_t* out) {
    if (!s || !pos || !nrm || !idx || !out || nv == 0 || nt == 0) return fail(MI355PT_E_INVALID, "bad mesh");
    if ((uv != nullptr) != (tri_tangent != nullptr)) return fail(MI355PT_E_INVALID, "uv and tri_tangent must be given together");
    for (size_t i = 0; i < (size_t)nt * 3; ++i) if (idx[i] >= nv) return fail(MI355PT_E_INVALID, "vertex index out of range");
    // a non-finite position would poison every box above it in the BVH: refuse it here rather than render garbage
    for (size_t i = 0; i < (size_t)nv * 3; ++i) if (!std::isfinite(pos[i])) return fail(MI355PT_E_INVALID, "non-finite vertex position");
    HostMesh m; m.n_vert = nv; m.n_tri = nt;
    m.pos.assign(pos, pos + (size_t)nv * 3);
    m.nrm.resize((size_t)nv * 3);
    for (uint32_t i = 0; i < nv; ++i) {   // Normal::new normalises and Normal::from renormalises (normal.rs:18-20,93-100)
        V3 n = norm3(norm3(V3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}));
        m.nrm[3 * i] = n.x; m.nrm[3 * i + 1] = n.y; m.nrm[3 * i + 2] = n.z;
    }
    if (uv) { m.uv.assign(uv, uv + (size_t)nv * 2); m.tangent.assign(tri_tangent, tri_tangent + (size_t)nt * 3); }
    m.idx.assign(idx, idx + (size_t)nt * 3);
    s->impl.meshes.push_back(std::move(m));
    *out = (uint32_t)s->impl.meshes.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_material(mi355pt_scene* s, const mi355pt_material_desc* d, uint32_t* out) {
    if (!s || !d || !out) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& im = s->impl;
    DevMaterial m{};
    std::string err;
    int rc;
    m.type = d->type;
    m.normal_tex = d->normal_tex; m.normal_flip_y = d->normal_flip_y; m.thin = d->thin;
    m.intensity = d->intensity; m.roughness = d->roughness; m.metallic = d->metallic; m.ior = d->ior;
    m.cc_ior = d->clearcoat_ior; m.cc_roughness = d->clearcoat_roughness; m.cc_thickness = d->clearcoat_thickness;
    m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu;
    m.intensity_avg = d->intensity;
    if (d->type == MI355PT_MAT_EMISSIVE && d->intensity_tex != MI355PT_NONE) {
        // FloatParameter::texture intensity (emissive_material.rs:55-56,69-76): the device reads it at the hit / sampled uv through the
        // material's metallic_tex slot; the light-pick weight uses ONE value, the texture at uv (0.5, 0.5), computed here with the device's
        // bilinear arithmetic (texture/sampler.rs:81-107: red channel of the gamma-encoded texel / 255)
        if (d->intensity_tex >= im.textures.size()) return fail(MI355PT_E_INVALID, "bad intensity texture id");
        m.metallic_tex = d->intensity_tex;
        const SceneImpl::Tex& t = im.textures[d->intensity_tex];
        const float u = std::fabs(0.5f - std::trunc(0.5f)), v = 1.0f - std::fabs(0.5f - std::trunc(0.5f));
        const float x = u * ((float)t.w - 1.0f), y = v * ((float)t.h - 1.0f);
        const uint32_t x0 = (uint32_t)std::floor(x), y0 = (uint32_t)std::floor(y), x1 = std::min(x0 + 1u, t.w - 1u), y1 = std::min(y0 + 1u, t.h - 1u);
        const float fx = x - (float)x0, fy = y - (float)y0;
        auto red = [&](uint32_t xx, uint32_t yy) { return (float)t.rgb[((size_t)yy * t.w + xx) * 3] / 255.0f; };
        const float top = red(x0, y0) * (1.0f - fx) + red(x1, y0) * fx, bottom = red(x0, y1) * (1.0f - fx) + red(x1, y1) * fx;
        m.intensity_avg = top * (1.0f - fy) + bottom * fy;
    }
    if (d->type == MI355PT_MAT_CLEARCOAT && d->clearcoat_thickness_tex != MI355PT_NONE) {
        if (d->clearcoat_thickness_tex >= im.textures.size()) return fail(MI355PT_E_INVALID, "bad clearcoat thickness texture id");
        m.cc_thickness_tex = d->clearcoat_thickness_tex;
    }
    if (d->type == MI355PT_MAT_GLASS || d->type == MI355PT_MAT_PLASTIC) {   // roughness: FloatParameter (glass_material.rs:42, plastic_material.rs:43)
        if (d->roughness_tex != MI355PT_NONE && d->roughness_tex >= im.textures.size()) return fail(MI355PT_E_INVALID, "bad roughness texture id");
        m.roughness_tex = d->roughness_tex;
    }
    if (d->type == MI355PT_MAT_SIMPLE_PBR || d->type == MI355PT_MAT_CLEARCOAT || d->type == MI355PT_MAT_METAL) {
        if ((d->metallic_tex != MI355PT_NONE && d->metallic_tex >= im.textures.size()) || (d->roughness_tex != MI355PT_NONE && d->roughness_tex >= im.textures.size()))
            return fail(MI355PT_E_INVALID, "bad metallic/roughness texture id");
        m.metallic_tex = d->type == MI355PT_MAT_METAL ? 0xffffffffu : d->metallic_tex; m.roughness_tex = d->roughness_tex;
    }
    if (d->normal_tex != MI355PT_NONE && d->normal_tex >= im.textures.size()) return fail(MI355PT_E_INVALID, "bad normal texture id");
    switch (d->type) {
        case MI355PT_MAT_LAMBERT:
            if ((rc = im.lower_spectrum(d->color, &m.color, true, &err))) return fail(rc, err);
            break;
        case MI355PT_MAT_EMISSIVE:
            // SpectrumParameter::Texture radiance (emissive_material.rs:48-79): an sRGB texture of any SpectrumType, looked up at the hit / sampled uv
            if ((rc = im.lower_spectrum(d->color, &m.color, 2, &err))) return fail(rc, "emissive radiance: " + err);
            break;
        case MI355PT_MAT_GLASS:
        case MI355PT_MAT_PLASTIC:
            if ((rc = im.lower_spectrum(d->eta, &m.eta, false, &err))) return fail(rc, "eta: " + err);
            if ((rc = im.lower_spectrum(d->color, &m.color, d->type == MI355PT_MAT_PLASTIC, &err))) return fail(rc, err);
            break;
        case MI355PT_MAT_CLEARCOAT:
            if ((rc = im.lower_spectrum(d->color, &m.color, true, &err))) return fail(rc, err);
            if ((rc = im.lower_spectrum(d->clearcoat_tint, &m.cc_tint, true, &err))) return fail(rc, "clearcoat tint: " + err);
            break;
        case MI355PT_MAT_SIMPLE_PBR:      // SimplePbrMaterial == the clearcoat material's base layer: thickness 0 takes exactly that path
            m.type = MT_CLEARCOAT; m.cc_thickness = 0.0f; m.cc_ior = 1.5f; m.cc_roughness = 0.0f;
            m.cc_tint.kind = SPK_CONSTANT; m.cc_tint.c[0] = 1.0f;
            if ((rc = im.lower_spectrum(d->color, &m.color, true, &err))) return fail(rc, err);
            break;
        case MI355PT_MAT_METAL:
            if ((rc = im.lower_spectrum(d->eta, &m.eta, false, &err))) return fail(rc, "eta: " + err);
            if ((rc = im.lower_spectrum(d->k, &m.cc_tint, false, &err))) return fail(rc, "k: " + err);
            break;
        default:
            return fail(MI355PT_E_INVALID, "material type not implemented on the device yet");
    }
    im.materials.push_back(m);
    *out = (uint32_t)im.materials.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_delta_light(mi355pt_scene* s, const mi355pt_light_desc* d) {
    if (!s || !d) return fail(MI355PT_E_INVALID, "null argument");
    if (d->kind < MI355PT_LIGHT_POINT || d->kind > MI355PT_LIGHT_DIRECTIONAL) return fail(MI355PT_E_INVALID, "bad light kind");
    SceneImpl& im = s->impl;
    DevMaterial m{};                        // hidden emissive material: carries the light's spectrum with intensity 1
    std::string err;
    int rc;
    m.type = MT_EMISSIVE; m.normal_tex = 0xffffffffu; m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu; m.intensity = 1.0f; m.intensity_avg = 1.0f;
    if ((rc = im.lower_spectrum(d->spectrum, &m.color, false, &err))) return fail(rc, "light spectrum: " + err);
    im.materials.push_back(m);
    HostDeltaLight hl{*d, (uint32_t)im.materials.size() - 1, (uint32_t)im.instances.size()};
    im.delta_lights.push_back(hl);
    return MI355PT_OK;
}
int mi355pt_scene_add_environment_light(mi355pt_scene* s, float intensity, const float* rgb, uint32_t w, uint32_t h, const float* l2w,
                                        uint32_t illuminant_lut) {
    if (!s || !rgb || !l2w || w == 0 || h == 0) return fail(MI355PT_E_INVALID, "bad environment light arguments");
    SceneImpl& im = s->impl;
    if (illuminant_lut >= im.luts.size()) return fail(MI355PT_E_INVALID, "bad illuminant LUT id");
    SceneImpl::HostEnv he;
    he.intensity = intensity; he.w = w; he.h = h; he.illuminant_lut = illuminant_lut;
    he.rgb.assign(rgb, rgb + (size_t)w * h * 3);
    std::memcpy(he.l2w, l2w, sizeof(float) * 16);
    im.envs.push_back(std::move(he));
    DevMaterial m{};                         // hidden emissive material: the integrated RgbIlluminantSpectrum, filled in at build()
    m.type = MT_EMISSIVE; m.normal_tex = 0xffffffffu; m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu; m.intensity = 1.0f; m.intensity_avg = 1.0f; m.color.kind = SPK_CONSTANT;
    im.materials.push_back(m);
    mi355pt_light_desc ld{}; ld.kind = LK_ENV; ld.intensity = intensity; std::memcpy(ld.local_to_world, l2w, sizeof(float) * 16);
    im.delta_lights.push_back(HostDeltaLight{ld, (uint32_t)im.materials.size() - 1, (uint32_t)im.instances.size(), (uint32_t)im.envs.size() - 1});
    return MI355PT_OK;
}
int mi355pt_scene_add_instance(mi355pt_scene* s, uint32_t geom, uint32_t mat, const float* l2w) {
    if (!s || !l2w) return fail(MI355PT_E_INVALID, "null argument");
    if (geom >= s->impl.meshes.size() || mat >= s->impl.materials.size()) return fail(MI355PT_E_INVALID, "bad geometry/material id");
    HostInstance hi; hi.geom = geom; hi.mat = mat; std::memcpy(hi.l2w, l2w, sizeof(float) * 16);
    s->impl.instances.push_back(hi);
    return MI355PT_OK;
}
int mi355pt_coat_albedo_table(float alpha, float r0, float* out) {
    if (!out || !(alpha >= 0.0f) || !(r0 >= 0.0f)) return fail(MI355PT_E_INVALID, "bad argument");
    coat_albedo_table(alpha, r0, out);
    return MI355PT_OK;
}
int mi355pt_scene_set_bvh_builder(mi355pt_scene* s, int mode) {
    if (!s) return fail(MI355PT_E_INVALID, "null argument");
    if (mode != MI355PT_BVH_AUTO && mode != MI355PT_BVH_HOST && mode != MI355PT_BVH_GPU) return fail(MI355PT_E_INVALID, "unknown BVH builder mode");
    s->impl.bvh_builder = mode;
    return MI355PT_OK;
}
int mi355pt_scene_build(mi355pt_scene* s, const mi355pt_camera* cam) {
    if (!s || !cam) return fail(MI355PT_E_INVALID, "null argument");
    std::string err;
    float cmf[470 * 4];
    cie_cmf4(cmf);
    int rc = s->impl.build(cam, cmf, &err);
    // the launch context belongs to the old build: another feature set launches other kernels (cached grid sizes), another device makes its
    // buffers foreign memory — get_launch_ctx makes a new one, on the build's device, at the next render
    delete s->ctx; s->ctx = nullptr;
    return rc ? fail(rc, err) : MI355PT_OK;
}

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


// ---------------- several GPUs of one node behind ONE call (single process) ----------------
// The reference calls the seam once from one process (renderer/src/main.rs:228).  mi355pt_scene_build_multi replicates the scene
// on every listed device (the working set is < 30 MB); mi355pt_render_multi deals the frame's 8x8 tiles round-robin to the devices
// (each launch on its own stream, concurrently), gathers the rank-local linear films onto the first device over xGMI peer copies
// and adds them there — the tile shards are disjoint, so the sum is exact and its order fixed — then resolves and copies out.
// No communicator is needed inside one process; the one-process-per-GPU path (bench.py, torch.distributed) reduces the same films
// with RCCL.
int mi355pt_scene_build_multi(mi355pt_scene* s, const mi355pt_camera* cam, int n_devices, const int* device_ids) {
    if (!s || !cam || !device_ids || n_devices < 1 || n_devices > 64) return fail(MI355PT_E_INVALID, "bad device list");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MI355PT_E_NO_DEVICE, "no HIP device: the product path requires a gfx950 GPU");
    for (int i = 0; i < n_devices; ++i) if (device_ids[i] < 0 || device_ids[i] >= ndev) return fail(MI355PT_E_INVALID, "device id out of range");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    free_parts(s->parts);
    int rc = MI355PT_OK;
    std::vector<MultiPart> parts((size_t)n_devices);
    for (int i = 0; i < n_devices && rc == MI355PT_OK; ++i) {
        MultiPart& m = parts[(size_t)i];
        m.device = device_ids[i];
        if (hipSetDevice(m.device) != hipSuccess) { rc = fail(MI355PT_E_DEVICE, "hipSetDevice failed"); break; }
        if (i == 0) m.scene = s;
        else {
            m.scene = new (std::nothrow) mi355pt_scene();
            if (!m.scene) { rc = fail(MI355PT_E_INVALID, "allocation failed"); break; }
            SceneImpl& d = m.scene->impl; const SceneImpl& o = s->impl;       // the description, not the lowered state
            d.table = o.table; d.luts = o.luts; d.textures = o.textures; d.meshes = o.meshes; d.materials = o.materials;
            d.instances = o.instances; d.envs = o.envs; d.delta_lights = o.delta_lights; d.bvh_builder = o.bvh_builder; d.lowering = o.lowering;
        }
        rc = mi355pt_scene_build(m.scene, cam);
        if (rc == MI355PT_OK && hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking) != hipSuccess) rc = fail(MI355PT_E_DEVICE, "hipStreamCreate failed");
        if (rc == MI355PT_OK && hipEventCreateWithFlags(&m.done, hipEventDisableTiming) != hipSuccess) rc = fail(MI355PT_E_DEVICE, "hipEventCreate failed");
        if (rc == MI355PT_OK && i > 0 && m.device != parts[0].device) {
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, parts[0].device, m.device);
            if (can) { (void)hipSetDevice(parts[0].device); (void)hipDeviceEnablePeerAccess(m.device, 0); (void)hipGetLastError(); }   // already enabled is fine
        }
    }
    (void)hipSetDevice(cur);
    if (rc != MI355PT_OK) { std::string keep = g_err; free_parts(parts); g_err = keep; return rc; }
    s->parts = std::move(parts);
    return MI355PT_OK;
}

int mi355pt_render_multi(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, float* out_rgb) {
    if (!s || !cam || !p || !out_rgb) return fail(MI355PT_E_INVALID, "null argument");
    if (s->parts.empty()) return fail(MI355PT_E_NOT_BUILT, "scene not built with mi355pt_scene_build_multi");
    if (p->shard_count > 1) return fail(MI355PT_E_INVALID, "mi355pt_render_multi shards the frame itself: pass shard_count 0 or 1");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "collect_stats is a single-device diagnostic");
    if (cam->width == 0 || cam->height == 0 || p->spp == 0) return fail(MI355PT_E_INVALID, "empty image or spp == 0");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    std::vector<MultiPart>& parts = s->parts;
    const uint32_t n = (uint32_t)parts.size();
    const size_t film = (size_t)cam->width * cam->height * 3, film_pad = (film + 3) / 4 * 4;
    int rc = MI355PT_OK;
    auto hip_ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == MI355PT_OK) rc = fail(MI355PT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); return e == hipSuccess; };
    // the shards: device i renders frame tiles i, i + n, i + 2 n, ...; its share of the film is tiles_of(i) * 192 floats
    auto tiles_of = [&](uint32_t i) { return shard_tile_count(cam->width, cam->height, i, n); };
    std::vector<size_t> stage_off(n, 0);
    size_t stage_total = 0;
    for (uint32_t i = 1; i < n; ++i) { stage_off[i] = stage_total; stage_total += (size_t)tiles_of(i) * 192u; }
    // 1. every device renders its tile shard into its own zeroed film, concurrently; a peer then packs its tiles and PUSHES the compact
    //    film (film / n bytes) into its own landing area on the first device, on its own stream: the n - 1 transfers overlap each other
    //    and the first device's rendering
    {
        MultiPart& r = parts[0];
        if (hip_ok(hipSetDevice(r.device), "hipSetDevice") && r.stage_floats < stage_total) {
            (void)hipFree(r.d_stage); r.d_stage = nullptr; r.stage_floats = 0;
            if (hip_ok(hipMalloc((void**)&r.d_stage, stage_total * sizeof(float)), "hipMalloc stage")) r.stage_floats = stage_total;
        }
    }
    for (uint32_t i = 0; i < n && rc == MI355PT_OK; ++i) {
        MultiPart& m = parts[i];
        if (!hip_ok(hipSetDevice(m.device), "hipSetDevice")) break;
        if (m.film_floats != film_pad) {
            (void)hipFree(m.d_film); (void)hipFree(m.d_out); m.d_film = m.d_out = nullptr; m.film_floats = 0;
            if (!hip_ok(hipMalloc((void**)&m.d_film, film_pad * sizeof(float)), "hipMalloc film")) break;
            if (i == 0 && !hip_ok(hipMalloc((void**)&m.d_out, film_pad * sizeof(float)), "hipMalloc out")) break;
            m.film_floats = film_pad;
        }
        const size_t pack = (size_t)tiles_of(i) * 192u;
        if (i > 0 && m.pack_floats < pack) {
            (void)hipFree(m.d_pack); m.d_pack = nullptr; m.pack_floats = 0;
            if (!hip_ok(hipMalloc((void**)&m.d_pack, std::max<size_t>(pack, 1) * sizeof(float)), "hipMalloc pack")) break;
            m.pack_floats = pack;
        }
        if (!hip_ok(hipMemsetAsync(m.d_film, 0, film_pad * sizeof(float), m.stream), "hipMemsetAsync")) break;
        mi355pt_params q = *p;
        q.shard_index = i; q.shard_count = n;
        if ((rc = mi355pt_render_accum_device(m.scene, cam, &q, 0, p->spp, m.d_film, (void*)m.stream, nullptr))) break;
        if (i > 0 && pack) {
            if (!hip_ok(launch_film_pack(m.d_film, cam->width, cam->height, i, n, tiles_of(i), m.d_pack, m.stream), "film pack")) break;
            if (!hip_ok(hipMemcpyPeerAsync(parts[0].d_stage + stage_off[i], parts[0].device, m.d_pack, m.device, pack * sizeof(float), m.stream), "hipMemcpyPeerAsync")) break;
        }
        hip_ok(hipEventRecord(m.done, m.stream), "hipEventRecord");
    }
    // 2. on the first device: each landed shard is written into the film (disjoint tiles: stores in a fixed order, exact and
    //    deterministic), then resolve and copy out
    if (rc == MI355PT_OK && hip_ok(hipSetDevice(parts[0].device), "hipSetDevice")) {
        MultiPart& r = parts[0];
        for (uint32_t i = 1; i < n && rc == MI355PT_OK; ++i) {
            if (!tiles_of(i)) continue;
            if (!hip_ok(hipStreamWaitEvent(r.stream, parts[i].done, 0), "hipStreamWaitEvent")) break;
            hip_ok(launch_film_unpack(r.d_film, cam->width, cam->height, i, n, tiles_of(i), r.d_stage + stage_off[i], r.stream), "film unpack");
        }
        if (rc == MI355PT_OK) rc = mi355pt_film_resolve_device(r.d_film, cam->width * cam->height, p->spp, r.d_out, (void*)r.stream);
        if (rc == MI355PT_OK) hip_ok(hipMemcpyAsync(out_rgb, r.d_out, film * sizeof(float), hipMemcpyDeviceToHost, r.stream), "hipMemcpyAsync");
        if (rc == MI355PT_OK) hip_ok(hipStreamSynchronize(r.stream), "hipStreamSynchronize");
    }
    if (rc != MI355PT_OK) for (MultiPart& m : parts) { (void)hipSetDevice(m.device); (void)hipStreamSynchronize(m.stream); }   // nothing of this call stays in flight
    (void)hipSetDevice(cur);
    return rc;
}

int mi355pt_scene_info(const mi355pt_scene* s, char* buf, size_t n) {
    if (!s || !buf || n == 0) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_INVALID, "scene not built");
    std::snprintf(buf, n, "%s", s->impl.info.c_str());
    return MI355PT_OK;
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
    HIP_TRY(hipMemcpy(out_rgb, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost));
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

// ---------------- denoiser (include/mi355pt_denoise.h) ----------------

void mi355pt_denoise_params_default(mi355pt_denoise_params* out) {
    if (!out) return;
    out->levels = 5; out->sigma_color = 1.0f; out->sigma_normal = 0.5f; out->sigma_albedo = 0.3f; out->albedo_eps = 0.01f;
}
size_t mi355pt_denoise_scratch_bytes(uint32_t width, uint32_t height) { return denoise_scratch_bytes(width, height); }

// every check of mi355pt_denoise_device / mi355pt_denoise that does not concern the scratch; host arithmetic only
static int denoise_check(const float* beauty, uint32_t spp_b, const float* albedo, uint32_t spp_a, const float* normal, uint32_t spp_n, uint32_t width,
                         uint32_t height, const mi355pt_denoise_params* dp, const float* out) {
    if (!beauty || !out || !dp) return fail(MI355PT_E_INVALID, "denoise: null beauty, output or params pointer");
    if (dp->levels < 1 || dp->levels > 8) return fail(MI355PT_E_INVALID, "denoise: levels must be 1 .. 8 (mi355pt_denoise_params_default fills the struct)");
    const float pos[4] = {dp->sigma_color, dp->sigma_normal, dp->sigma_albedo, dp->albedo_eps};
    for (float v : pos)
        if (!(std::isfinite(v) && v > 0.0f)) return fail(MI355PT_E_INVALID, "denoise: sigma_color, sigma_normal, sigma_albedo and albedo_eps must be finite and > 0");
    if (spp_b == 0 || (albedo && spp_a == 0) || (normal && spp_n == 0)) return fail(MI355PT_E_INVALID, "denoise: spp of a given buffer is 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "denoise: zero width or height");
    if (denoise_grid_blocks(width, height) == 0 || denoise_scratch_bytes(width, height) == 0) return fail(MI355PT_E_INVALID, "denoise: frame too large");
    if (out == beauty || out == albedo || out == normal) return fail(MI355PT_E_INVALID, "denoise: the output must not be one of the inputs");
    return MI355PT_OK;
}

int mi355pt_denoise_device(const float* d_beauty, uint32_t spp_b, const float* d_albedo, uint32_t spp_a, const float* d_normal, uint32_t spp_n,
                           uint32_t width, uint32_t height, const mi355pt_denoise_params* dp, void* d_scratch, size_t scratch_bytes, float* d_out,
                           void* hip_stream) {
    int rc = denoise_check(d_beauty, spp_b, d_albedo, spp_a, d_normal, spp_n, width, height, dp, d_out);
    if (rc) return rc;
    if (!d_scratch || scratch_bytes < denoise_scratch_bytes(width, height)) return fail(MI355PT_E_INVALID, "denoise: scratch missing or smaller than mi355pt_denoise_scratch_bytes");
    if (((uintptr_t)d_scratch & 15u) != 0) return fail(MI355PT_E_INVALID, "denoise: scratch is not 16-byte aligned");
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
    HIP_TRY(d_b.alloc(n));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    HIP_TRY(hipMemcpy(d_b.p, beauty, n * sizeof(float), hipMemcpyHostToDevice));
    if (albedo) { HIP_TRY(d_a.alloc(n)); HIP_TRY(hipMemcpy(d_a.p, albedo, n * sizeof(float), hipMemcpyHostToDevice)); }
    if (normal) { HIP_TRY(d_n.alloc(n)); HIP_TRY(hipMemcpy(d_n.p, normal, n * sizeof(float), hipMemcpyHostToDevice)); }
    if ((rc = mi355pt_denoise_device(d_b.p, spp_b, albedo ? d_a.p : nullptr, spp_a, normal ? d_n.p : nullptr, spp_n, width, height, dp, d_scratch.p,
                                     scratch_bytes, d_out.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost));      // (synchronises the default stream)
    return MI355PT_OK;
}

// ---------------- variance-guided denoiser (include/mi355pt_denoise_var.h) ----------------

void mi355pt_denoise_var_params_default(mi355pt_denoise_var_params* out) {
    if (!out) return;
    out->levels = 5; out->sigma_lum = 4.0f; out->sigma_normal = 0.5f; out->sigma_albedo = 0.3f; out->albedo_eps = 0.01f; out->lum_eps = 1e-4f;
}
size_t mi355pt_denoise_var_scratch_bytes(uint32_t width, uint32_t height) { return denoise_var_scratch_bytes(width, height); }

// every check of mi355pt_denoise_var_device / mi355pt_denoise_var that does not concern the scratch; host arithmetic only
static int denoise_var_check(const float* beauty, const float* half, uint32_t spp_b, const uint32_t* tile_spp, const float* albedo, uint32_t spp_a,
                             const float* normal, uint32_t spp_n, uint32_t width, uint32_t height, const mi355pt_denoise_var_params* dp, const float* out) {
    if (!beauty || !half || !out || !dp) return fail(MI355PT_E_INVALID, "denoise_var: null beauty, half film, output or params pointer");
    if (dp->levels < 1 || dp->levels > 8) return fail(MI355PT_E_INVALID, "denoise_var: levels must be 1 .. 8 (mi355pt_denoise_var_params_default fills the struct)");
    const float pos[5] = {dp->sigma_lum, dp->sigma_normal, dp->sigma_albedo, dp->albedo_eps, dp->lum_eps};
    for (float v : pos)
        if (!(std::isfinite(v) && v > 0.0f)) return fail(MI355PT_E_INVALID, "denoise_var: sigma_lum, sigma_normal, sigma_albedo, albedo_eps and lum_eps must be finite and > 0");
    if (!tile_spp && (spp_b == 0 || (spp_b & 1u) != 0u)) return fail(MI355PT_E_INVALID, "denoise_var: spp_beauty must be even and > 0 (the half film holds the first spp_beauty / 2 samples)");
    if (tile_spp && spp_b != 0) return fail(MI355PT_E_INVALID, "denoise_var: spp_beauty must be 0 when tile counts are given");
    if ((albedo && spp_a == 0) || (normal && spp_n == 0)) return fail(MI355PT_E_INVALID, "denoise_var: spp of a given buffer is 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, "denoise_var: zero width or height");
    if (denoise_grid_blocks(width, height) == 0 || denoise_var_scratch_bytes(width, height) == 0) return fail(MI355PT_E_INVALID, "denoise_var: frame too large");
    if (out == beauty || out == half || out == albedo || out == normal || (const void*)out == (const void*)tile_spp)
        return fail(MI355PT_E_INVALID, "denoise_var: the output must not be one of the inputs");
    return MI355PT_OK;
}

int mi355pt_denoise_var_device(const float* d_beauty, const float* d_half, uint32_t spp_b, const uint32_t* d_tile_spp, const float* d_albedo, uint32_t spp_a,
                               const float* d_normal, uint32_t spp_n, uint32_t width, uint32_t height, const mi355pt_denoise_var_params* dp, void* d_scratch,
                               size_t scratch_bytes, float* d_out, void* hip_stream) {
    int rc = denoise_var_check(d_beauty, d_half, spp_b, d_tile_spp, d_albedo, spp_a, d_normal, spp_n, width, height, dp, d_out);
    if (rc) return rc;
    if (!d_scratch || scratch_bytes < denoise_var_scratch_bytes(width, height)) return fail(MI355PT_E_INVALID, "denoise_var: scratch missing or smaller than mi355pt_denoise_var_scratch_bytes");
    if (((uintptr_t)d_scratch & 15u) != 0) return fail(MI355PT_E_INVALID, "denoise_var: scratch is not 16-byte aligned");
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
    HIP_TRY(d_b.alloc(n));
    HIP_TRY(d_h.alloc(n));
    HIP_TRY(d_out.alloc(n));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    HIP_TRY(hipMemcpy(d_b.p, beauty, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_h.p, half_film, n * sizeof(float), hipMemcpyHostToDevice));
    if (tile_spp) { HIP_TRY(d_t.alloc(n_tiles)); HIP_TRY(hipMemcpy(d_t.p, tile_spp, n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice)); }
    if (albedo) { HIP_TRY(d_a.alloc(n)); HIP_TRY(hipMemcpy(d_a.p, albedo, n * sizeof(float), hipMemcpyHostToDevice)); }
    if (normal) { HIP_TRY(d_n.alloc(n)); HIP_TRY(hipMemcpy(d_n.p, normal, n * sizeof(float), hipMemcpyHostToDevice)); }
    if ((rc = mi355pt_denoise_var_device(d_b.p, d_h.p, spp_b, tile_spp ? d_t.p : nullptr, albedo ? d_a.p : nullptr, spp_a, normal ? d_n.p : nullptr, spp_n, width,
                                         height, dp, d_scratch.p, scratch_bytes, d_out.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost));      // (synchronises the default stream)
    return MI355PT_OK;
}

// ---------------- adaptive sampling (include/mi355pt_adaptive.h) ----------------

size_t mi355pt_adaptive_scratch_bytes(uint32_t width, uint32_t height) { return adaptive_scratch_bytes(width, height); }

static int adaptive_check_params(const mi355pt_adaptive_params* ap) {
    if (!ap) return fail(MI355PT_E_INVALID, "adaptive: null params pointer");
    if (!(std::isfinite(ap->threshold) && ap->threshold > 0.0f)) return fail(MI355PT_E_INVALID, "adaptive: threshold must be finite and > 0 (it has no default)");
    if (!(std::isfinite(ap->dark_eps) && ap->dark_eps > 0.0f)) return fail(MI355PT_E_INVALID, "adaptive: dark_eps must be finite and > 0");
    if (ap->min_spp < 2u || (ap->min_spp & (ap->min_spp - 1u)) != 0u) return fail(MI355PT_E_INVALID, "adaptive: min_spp must be a power of two >= 2");
    return MI355PT_OK;
}
static int adaptive_check_scratch(uint32_t width, uint32_t height, const void* d_scratch, size_t scratch_bytes) {
    if (width == 0 || height == 0 || adaptive_tile_count(width, height) == 0u) return fail(MI355PT_E_INVALID, "adaptive: zero width or height, or a frame of 2^31 tiles or more");
    if (!d_scratch || scratch_bytes < adaptive_scratch_bytes(width, height)) return fail(MI355PT_E_INVALID, "adaptive: scratch missing or smaller than mi355pt_adaptive_scratch_bytes");
    if (((uintptr_t)d_scratch & 3u) != 0) return fail(MI355PT_E_INVALID, "adaptive: scratch is not 4-byte aligned");
    return MI355PT_OK;
}

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

// every check of the two drivers that does not concern the device buffers
static int adaptive_check_render(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const mi355pt_adaptive_params* ap) {
    int rc = check_tiles_args(s, cam, p);
    if (rc) return rc;
    if ((rc = adaptive_check_params(ap))) return rc;
    if ((p->spp & (p->spp - 1u)) != 0u || p->spp < ap->min_spp) return fail(MI355PT_E_INVALID, "adaptive: spp (the maximum) must be a power of two >= min_spp");
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
    HIP_TRY(hipMemcpy(out_rgb, d_film.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (out_tile_spp) HIP_TRY(hipMemcpy(out_tile_spp, d_spp.p, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MI355PT_OK;
}

// ---------------- G-buffer pass (include/mi355pt_gbuffer.h) ----------------

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

// one launch of a sample range (arguments checked), after launch_range
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
    unsigned* d_counter = lc->d_counters + slot;
    DevStats* d_stats = lc->d_stats + slot;
    HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(unsigned), stream));
    if (stats) HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(DevStats), stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (stats) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, stream)); }
    const GbufferFilms gf{films->albedo, films->shading_normal, films->position, films->hit};
    HIP_TRY(launch_gbuffer(s->impl.dev, dc, plan.params, illuminant_lut, lc->d_hash, gf, d_counter, stats ? d_stats : nullptr, s->impl.features, plan.grid,
                           stream));
    if (stats) {
        HIP_TRY(hipEventRecord(e1, stream));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        std::memset(stats, 0, sizeof(*stats));
        stats->kernel_ms = ms; stats->launches = 1;
        DevStats h;
        HIP_TRY(hipMemcpy(&h, d_stats, sizeof(h), hipMemcpyDeviceToHost));
        copy_stats(h, stats);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return MI355PT_OK;   // stats == NULL: fully asynchronous on `stream`
}

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
    const mi355pt_gbuffer_films dev{host[0] ? d_acc[0].p : nullptr, host[1] ? d_acc[1].p : nullptr, host[2] ? d_acc[2].p : nullptr,
                                    host[3] ? d_acc[3].p : nullptr};
    if ((rc = mi355pt_render_gbuffer_accum_device(s, cam, p, illuminant_lut, 0u, p->spp, &dev, nullptr, stats))) return rc;
    for (int i = 0; i < 4; ++i) {
        if (!host[i]) continue;
        // albedo: Sensor::to_rgb with NoneToneMap; the other films: sum / spp, raw (the resolve of the shading-normal kind)
        if ((rc = mi355pt_aov_resolve_device(i == 0 ? MI355PT_AOV_ALBEDO : MI355PT_AOV_SHADING_NORMAL, d_acc[i].p, cam->width * cam->height, p->spp,
                                             d_res.p, nullptr))) return rc;
        HIP_TRY(hipMemcpy(host[i], d_res.p, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return MI355PT_OK;
}

int mi355pt_quantize_u8(const float* rgb, size_t n, uint8_t* out) {
    if (!rgb || !out) return fail(MI355PT_E_INVALID, "null argument");
    for (size_t i = 0; i < n; ++i) {   // Rust `as u8`: saturating, NaN -> 0 (renderer.rs:141-143)
        float v = rgb[i] * 255.0f;
        out[i] = std::isnan(v) ? 0 : (v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (uint8_t)v));
    }
    return MI355PT_OK;
}

}  // extern "C"
