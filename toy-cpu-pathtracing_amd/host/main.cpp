// mi355pt — command line mirroring renderer/src/main.rs:20-140 (clap flags, defaults and flow), with
// RendererImage::render running on the MI355X through libmi355pt.so instead of the rayon pixel loop.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include <hip/hip_runtime_api.h>   // --denoise, --denoise-variance, --adaptive-threshold, --temporal-frames, --half-res, --tone-map, --auto-exposure and --robust-buckets: the films of those paths stay on the device (hipMalloc / hipMemcpy / hipFree, no kernels here)

#include "scenes.hpp"

using namespace renderer;

struct Args {   // main.rs:20-53
    uint32_t scene = 0, spp = 64, seed = 0, width = 800, height = 600, max_depth = 16;
    std::string filter = "box", sampler = "random", renderer = "normal", output = "output.png";
    // not in the reference's CLI: the coat-albedo table option (mi355pt_params.albedo_lut) and the number of GPUs of this node to shard the frame over
    bool albedo_lut = false; int gpus = 1;
    // not in the reference's CLI either: the a-trous denoiser (mi355pt_denoise.h) behind a path renderer, and the spp of its two guide films
    bool denoise = false; uint32_t denoise_guide_spp = 64;
    // and the variance-guided one (mi355pt_denoise_var.h), which takes the film and a half film instead; 0 = its default sigma_lum
    bool denoise_variance = false; float denoise_sigma_lum = 0.0f;
    // nor is adaptive sampling (mi355pt_adaptive.h): --spp becomes the maximum.  The threshold has no default (0 = not adaptive).
    // dark_eps 1e-3 is a CHOICE, not a measurement: a thousandth of the radiance of a mid-grey pixel, so that black pixels neither divide
    // by zero nor dominate a tile's estimate
    float adaptive_threshold = 0.0f, adaptive_dark_eps = 1e-3f; uint32_t adaptive_min_spp = 16; std::string spp_map;
    // nor the G-buffer pass (mi355pt_gbuffer.h): with a denoise flag, the two guide films from ONE launch of it instead of two AOV launches
    bool fused_guides = false;
    // nor temporal accumulation (mi355pt_temporal.h): N frames, frame k with seed + k from position + k * step, each reprojected into the next
    bool temporal = false; uint32_t temporal_frames = 0; bool camera_step_given = false; float camera_step[3] = {0.0f, 0.0f, 0.0f};
    bool camera_move_given = false; std::string camera_move = "rebuild";   // --camera-move rebuild|rebase: how the frames of --temporal-frames follow --camera-step
    // and its rectified form (mi355pt_temporal_rectify.h): the history is first scaled to the current frame's local mean; radius and gamma not given = its defaults
    bool temporal_rectify = false, temporal_rectify_radius_given = false, temporal_rectify_gamma_given = false;
    uint32_t temporal_rectify_radius = 0; float temporal_rectify_gamma = 0.0f;
    // nor guided half-resolution rendering (mi355pt_upsample.h): the paths traced at width / 2 x height / 2, the frame rebuilt through both G-buffers;
    // albedo demodulation is off by default (profiles/upsample_quality.json: it does not win on both measured scenes)
    bool half_res = false, half_res_albedo = false;
    // nor the display stage (mi355pt_display.h): a tone curve other than the reference's Reinhard, and an exposure metered from the frame's
    // histogram instead of the constant 1 (--temporal-frames: every frame metered with the previous frame's record).  Not given = the defaults
    std::string tone_map; bool white_given = false; float white = 0.0f;
    bool auto_exposure = false, exposure_key_given = false, exposure_adapt_given = false, exposure_trim_given = false;
    float exposure_key = 0.0f, exposure_adapt = 0.0f; uint32_t exposure_trim[2] = {0, 0};
    // nor the bloom stage (mi355pt_bloom.h): between the meter and the tone curve of whatever device path renders the frame.  Not given = the
    // defaults (six levels, energy-conserving: base = 1 - intensity, no threshold); --bloom-additive: base 1 and, unless given, a threshold of 1
    bool bloom = false, bloom_additive = false, bloom_no_firefly = false;
    bool bloom_levels_given = false, bloom_threshold_given = false, bloom_knee_given = false, bloom_scatter_given = false, bloom_intensity_given = false;
    uint32_t bloom_levels = 0; float bloom_threshold = 0.0f, bloom_knee = 0.0f, bloom_scatter = 0.0f, bloom_intensity = 0.0f;
    // nor the robust film (mi355pt_robust.h): --spp rendered as K buckets of --spp / K consecutive samples, combined per pixel by a trimmed
    // mean of the bucket means (0 = off).  Mode and scale not given = mi355pt_robust_params_default: GMON, 1
    uint32_t robust_buckets = 0; bool robust_given = false; std::string robust_mode; bool robust_scale_given = false; float robust_scale = 0.0f;
    // nor moving instances of the built scene (mi355pt_instances.h): --instance-transform ID:tx,ty,tz[:ry_deg[:sx,sy,sz]], repeatable — the
    // scene is built as described with those instances marked dynamic, then each takes T . R_y . S . local_to_world on the device before the
    // frame.  --instance-rebuild-above 0 (the library's default): never build again because of the tree's SAH cost
    struct InstanceTransform { uint32_t id; float t[3]; float ry_deg; float s[3]; };
    std::vector<InstanceTransform> instance_transforms; bool instance_rebuild_given = false; float instance_rebuild_above = 0.0f;
    // nor object motion vectors (mi355pt_motion.h): --instance-step ID:tx,ty,tz[:ry_deg], repeatable, with --temporal-frames — in frame k the
    // instance's local_to_world is the scene's with T . R_y applied k times (the way --camera-step moves the camera); the instances are marked
    // dynamic before the build and moved on the device between the frames, and the accumulation is the motion-aware one
    std::vector<InstanceTransform> instance_steps;
    // nor edits of lights and materials of the built scene (mi355pt_edit.h), with --temporal-frames: --light-step ID:dx,dy,dz[:gain] (each frame
    // translates delta light ID and multiplies its intensity by gain), --emitter-gain MAT:g (each frame multiplies the emissive material's
    // intensity by g), --env-yaw-step DEG (each frame turns every environment light by DEG degrees about +y), and --scene-edit inplace|rebuild:
    // mi355pt_scene_edit alone, or followed by mi355pt_scene_build of the edited description (the default, the precedent of --camera-move)
    struct LightStep { uint32_t id; float d[3]; float gain; };
    struct EmitterGain { uint32_t mat; float gain; };
    std::vector<LightStep> light_steps; std::vector<EmitterGain> emitter_gains; bool env_yaw_given = false; float env_yaw_step = 0.0f;
    bool scene_edit_given = false; std::string scene_edit = "rebuild";
    bool editing() const { return !light_steps.empty() || !emitter_gains.empty() || env_yaw_given; }
    // nor deforming meshes of the built scene (mi355pt_deform.h): --mesh-wave GEOM:amp,wavelength[,phase_step], repeatable — the scene is
    // built as described, then every vertex of mesh GEOM takes y += amp sin(2 pi x / wavelength + phase_step) with area-weighted vertex
    // normals recomputed on the host, applied on the device before the frame.  --instance-rebuild-above applies to it
    struct MeshWave { uint32_t geom; float amp, wavelength, phase_step; };
    std::vector<MeshWave> mesh_waves;
    // nor per-pixel motion vectors (mi355pt_flow.h): --flow with --temporal-frames — every frame marks the scene, takes its moves (--camera-step,
    // --instance-step, --mesh-wave, any mix) in place, and accumulates through the flow pass's records; frame k of --mesh-wave then deforms the
    // ORIGINAL vertices with phase k * phase_step
    bool flow = false;
    // nor a sample budget by reprojected history (mi355pt_budget.h): --temporal-budget TARGET with --temporal-frames — every frame probes where its
    // history will be missing, renders --spp samples everywhere and up to --temporal-budget-max-spp (8 x --spp) on the tiles that start over
    bool temporal_budget = false, temporal_budget_max_given = false; float temporal_budget_target = 0.0f; uint32_t temporal_budget_max_spp = 0;
};

// the positions of a mesh under a wave along x that displaces y (local space), in double and rounded to float
std::vector<float> waved_positions(const Args::MeshWave& w, const std::vector<float>& pos, double phase) {
    std::vector<float> out(pos);
    for (size_t v = 0; v * 3 < pos.size(); ++v)
        out[3 * v + 1] = (float)((double)pos[3 * v + 1] + (double)w.amp * std::sin(2.0 * 3.14159265358979323846 * (double)pos[3 * v] / (double)w.wavelength + phase));
    return out;
}
std::vector<float> waved_positions(const Args::MeshWave& w, const std::vector<float>& pos) { return waved_positions(w, pos, (double)w.phase_step); }

// T . R_y . S . local_to_world (column-major): T R S composed in double and rounded to float, the product in double and rounded to float
void instance_transform_matrix(const Args::InstanceTransform& it, const float* l2w, float* out) {
    const double a = (double)it.ry_deg * (3.14159265358979323846 / 180.0), c = std::cos(a), s = std::sin(a);
    const double rot[3][3] = {{c, 0.0, s}, {0.0, 1.0, 0.0}, {-s, 0.0, c}};
    float x[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 1}};                    // row-major
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) x[r][k] = (float)(rot[r][k] * (double)it.s[k]); x[r][3] = it.t[r]; }
    for (int col = 0; col < 4; ++col) for (int r = 0; r < 4; ++r) {
        double v = 0.0;
        for (int k = 0; k < 4; ++k) v += (double)x[r][k] * (double)l2w[4 * col + k];
        out[4 * col + r] = (float)v;
    }
}

// --denoise: the beauty film at --spp, the albedo and shading-normal films at --denoise-guide-spp (converged guides cost a few percent of
// the frame; guides as noisy as the frame hurt), mi355pt_denoise_device, then Sensor::to_rgb on the result as a film with spp 1.
// Everything stays on the device until the resolved frame is copied into `pixels`.  Returns the device seconds of the beauty launch.
struct DeviceFilm {
    float* p = nullptr;
    explicit DeviceFilm(size_t bytes) {
        if (hipMalloc((void**)&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) throw std::runtime_error("mi355pt: device allocation failed");
    }
    ~DeviceFilm() { (void)hipFree(p); }
    DeviceFilm(const DeviceFilm&) = delete;
    DeviceFilm& operator=(const DeviceFilm&) = delete;
};
// The last step of every device path below.  Without --tone-map and --auto-exposure it IS mi355pt_film_resolve_device, the call this file
// made before the display stage existed.  With either, mi355pt_display_device: the chosen curve, sRGB, and — with --auto-exposure — the
// exposure of a record that mi355pt_display_meter_device wrote: the loops of --temporal-frames meter every frame's accumulated film with
// the previous frame's record (meter()), every other path meters the film it hands to resolve() there, with no previous record.
// With --bloom, resolve() first meters the UN-bloomed film (the glare does not feed the exposure), then mi355pt_bloom_device with that record
// into a buffer of the stage's own — the film it was handed, an accumulated history among them, is never written —, and what follows takes
// that buffer as a film of spp 1.
struct DisplayStage {
    bool on = false, auto_exposure = false, have_record = false, bloom_on = false;
    mi355pt_display_params dp{};
    mi355pt_bloom_params bp{};
    uint32_t* record = nullptr;
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    float* bloom_out = nullptr;
    void* bloom_scratch = nullptr;
    size_t bloom_out_bytes = 0, bloom_scratch_bytes = 0;
    void release() {      // (called in main: no HIP call from a static destructor)
        (void)hipFree(record); (void)hipFree(scratch); (void)hipFree(bloom_out); (void)hipFree(bloom_scratch);
        record = nullptr; scratch = nullptr; scratch_bytes = 0; bloom_out = nullptr; bloom_scratch = nullptr; bloom_out_bytes = bloom_scratch_bytes = 0;
    }
    static void grow(void** p, size_t* have, size_t need) {
        if (need <= *have) return;
        (void)hipFree(*p); *p = nullptr; *have = 0;
        if (hipMalloc(p, need) != hipSuccess) throw std::runtime_error("mi355pt: device allocation failed");
        *have = need;
    }
    // the bloomed film of `film`, spp 1, in the stage's own buffer
    const float* bloomed(const float* film, uint32_t width, uint32_t height, uint32_t spp) {
        if (on && auto_exposure && !have_record) meter(film, width, height, spp);
        grow((void**)&bloom_out, &bloom_out_bytes, (size_t)width * height * 3 * sizeof(float));
        grow(&bloom_scratch, &bloom_scratch_bytes, mi355pt_bloom_scratch_bytes(width, height, bp.levels));
        check(mi355pt_bloom_device(film, width, height, spp, &bp, on && auto_exposure ? record : nullptr, bloom_scratch, bloom_scratch_bytes, bloom_out, nullptr),
              "mi355pt_bloom_device");
        return bloom_out;
    }
    void meter(const float* film, uint32_t width, uint32_t height, uint32_t spp) {
        if (!on || !auto_exposure) return;
        const size_t need = mi355pt_display_scratch_bytes(width, height);
        if (!record && hipMalloc((void**)&record, MI355PT_DISPLAY_RECORD_WORDS * sizeof(uint32_t)) != hipSuccess) throw std::runtime_error("mi355pt: device allocation failed");
        if (need > scratch_bytes) {
            (void)hipFree(scratch); scratch = nullptr; scratch_bytes = 0;
            if (hipMalloc(&scratch, need) != hipSuccess) throw std::runtime_error("mi355pt: device allocation failed");
            scratch_bytes = need;
        }
        check(mi355pt_display_meter_device(film, width, height, spp, &dp, have_record ? record : nullptr, scratch, scratch_bytes, record, nullptr, nullptr),
              "mi355pt_display_meter_device");
        have_record = true;
    }
    void resolve(const float* film, uint32_t width, uint32_t height, uint32_t spp, float* rgb) {
        if (bloom_on) { film = bloomed(film, width, height, spp); spp = 1; }
        if (!on) { check(mi355pt_film_resolve_device(film, width * height, spp, rgb, nullptr), "mi355pt_film_resolve_device"); return; }
        if (auto_exposure && !have_record) meter(film, width, height, spp);
        check(mi355pt_display_device(film, width, height, spp, &dp, auto_exposure ? record : nullptr, rgb, nullptr), "mi355pt_display_device");
        if (auto_exposure) {
            uint32_t r[MI355PT_DISPLAY_RECORD_WORDS];
            float e[3];
            if (hipMemcpy(r, record, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the exposure record back failed");
            std::memcpy(e, r, sizeof e);
            std::printf("(auto-exposure: E %.6g, target %.6g, mean luminance %.6g; %u pixels metered, %u below and %u above the range)\n", e[0], e[1], e[2], r[3], r[4], r[5]);
        }
    }
};
static DisplayStage display_stage;      // configured once in main, before any render path runs

// --tone-map / --auto-exposure on a plain path render (no filter, no accumulation): the film at --spp on the device, then the display stage.
// Returns the device seconds of the beauty launch.
static double render_displayed(const Scene& scene, const Camera& camera, mi355pt_params p, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const size_t film_bytes = (size_t)cam.width * cam.height * 3 * sizeof(float);
    DeviceFilm film(film_bytes), rgb(film_bytes);
    mi355pt_stats st{};
    check(mi355pt_render_accum_device(scene.raw(), &cam, &p, 0, p.spp, film.p, nullptr, &st), "mi355pt_render_accum_device");
    display_stage.resolve(film.p, cam.width, cam.height, p.spp, rgb.p);
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    return st.kernel_ms * 1e-3;
}

static void render_guides(const Scene& scene, const mi355pt_camera& cam, mi355pt_params g, uint32_t guide_spp, bool fused, float* d_albedo, float* d_normal);
static mi355pt_denoise_var_params denoise_var_params(float sigma_lum);

// --robust-buckets K: the frame as K bucket films (mi355pt_render_buckets_device), then mi355pt_robust_combine_device.  Plain: the single
// output, a film with spp 1, to the display stage or the resolve.  --denoise: the single output as the beauty film with spp 1.
// --denoise-variance: the pair output as (beauty, half) with spp 2.  Prints the share of pixels trimmed and the mean trim count.  Returns
// the device seconds of the K bucket launches.
static double render_robust(const Scene& scene, const Camera& camera, mi355pt_params p, const Args& a, const mi355pt_robust_params& rp, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const uint32_t n_pixels = cam.width * cam.height, K = a.robust_buckets, guide_spp = a.denoise_guide_spp;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), trim_bytes = (size_t)n_pixels * 2;
    const bool pair = a.denoise_variance;
    DeviceFilm buckets(film_bytes * K), theta(film_bytes), half(pair ? film_bytes : 4), trim(trim_bytes), rgb(film_bytes);
    mi355pt_stats st{};
    check(mi355pt_render_buckets_device(scene.raw(), &cam, &p, K, buckets.p, nullptr, &st), "mi355pt_render_buckets_device");
    check(mi355pt_robust_combine_device(buckets.p, K, p.spp / K, cam.width, cam.height, &rp, theta.p, pair ? half.p : nullptr, (uint8_t*)trim.p, nullptr),
          "mi355pt_robust_combine_device");
    if (a.denoise || a.denoise_variance) {
        const size_t scratch_bytes = pair ? mi355pt_denoise_var_scratch_bytes(cam.width, cam.height) : mi355pt_denoise_scratch_bytes(cam.width, cam.height);
        DeviceFilm albedo(film_bytes), normal(film_bytes), out(film_bytes), scratch(scratch_bytes);
        render_guides(scene, cam, p, guide_spp, a.fused_guides, albedo.p, normal.p);
        if (pair) {
            const mi355pt_denoise_var_params dp = denoise_var_params(a.denoise_sigma_lum);
            check(mi355pt_denoise_var_device(theta.p, half.p, 2, nullptr, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp, scratch.p, scratch_bytes,
                                             out.p, nullptr), "mi355pt_denoise_var_device");
        } else {
            mi355pt_denoise_params dp;
            mi355pt_denoise_params_default(&dp);
            check(mi355pt_denoise_device(theta.p, 1, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp, scratch.p, scratch_bytes, out.p, nullptr), "mi355pt_denoise_device");
        }
        display_stage.resolve(out.p, cam.width, cam.height, 1, rgb.p);
    } else {
        display_stage.resolve(theta.p, cam.width, cam.height, 1, rgb.p);
    }
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    std::vector<uint8_t> t(trim_bytes);
    if (hipMemcpy(t.data(), trim.p, trim_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the trim counts back failed");
    uint64_t trimmed = 0, total = 0;
    for (uint32_t i = 0; i < n_pixels; ++i) {
        const uint32_t ti = pair ? (uint32_t)t[2 * i] + t[2 * i + 1] : t[2 * i];
        trimmed += ti != 0; total += ti;
    }
    std::printf("(robust film: %u buckets of %u spp%s; %.2f %% of the pixels trimmed, mean trim count %.3f of at most %u)\n", K, p.spp / K,
                pair ? ", even and odd sets" : "", 100.0 * (double)trimmed / n_pixels, (double)total / n_pixels / (pair ? 2.0 : 1.0), (pair ? K / 2 : K) / 2 - 1);
    return st.kernel_ms * 1e-3;
}

// The two guide films of the denoise paths, guide_spp samples each into zeroed device films: two launches of the AOV kernel, or — `fused`,
// --fused-guides — one launch of the G-buffer pass, whose two films then come from the same primary rays (the albedo film is the same bits
// either way; the shading-normal film sees the albedo renderer's sub-pixel positions instead of its own)
static void render_guides(const Scene& scene, const mi355pt_camera& cam, mi355pt_params g, uint32_t guide_spp, bool fused, float* d_albedo, float* d_normal) {
    g.spp = guide_spp;
    if (fused) {
        const mi355pt_gbuffer_films films{d_albedo, d_normal, nullptr, nullptr};
        check(mi355pt_render_gbuffer_accum_device(scene.raw(), &cam, &g, scene.d65_lut(), 0, guide_spp, &films, nullptr, nullptr), "mi355pt_render_gbuffer_accum_device");
        return;
    }
    check(mi355pt_render_aov_accum_device(scene.raw(), &cam, &g, MI355PT_AOV_ALBEDO, scene.d65_lut(), 0, guide_spp, d_albedo, nullptr, nullptr), "mi355pt_render_aov_accum_device");
    check(mi355pt_render_aov_accum_device(scene.raw(), &cam, &g, MI355PT_AOV_SHADING_NORMAL, scene.d65_lut(), 0, guide_spp, d_normal, nullptr, nullptr), "mi355pt_render_aov_accum_device");
}
static double render_denoised(const Scene& scene, const Camera& camera, mi355pt_params p, uint32_t guide_spp, bool fused, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const uint32_t n_pixels = cam.width * cam.height;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), scratch_bytes = mi355pt_denoise_scratch_bytes(cam.width, cam.height);
    DeviceFilm beauty(film_bytes), albedo(film_bytes), normal(film_bytes), out(film_bytes), rgb(film_bytes), scratch(scratch_bytes);
    mi355pt_stats st{};
    check(mi355pt_render_accum_device(scene.raw(), &cam, &p, 0, p.spp, beauty.p, nullptr, &st), "mi355pt_render_accum_device");
    render_guides(scene, cam, p, guide_spp, fused, albedo.p, normal.p);
    mi355pt_denoise_params dp;
    mi355pt_denoise_params_default(&dp);
    check(mi355pt_denoise_device(beauty.p, p.spp, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp, scratch.p, scratch_bytes, out.p, nullptr), "mi355pt_denoise_device");
    display_stage.resolve(out.p, cam.width, cam.height, 1, rgb.p);
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    return st.kernel_ms * 1e-3;
}

// --denoise-variance: the half film H = [0, spp / 2), the film F = H + [spp / 2, spp) — the pair the adaptive driver keeps, here at one
// count for the whole frame —, the guide films as for --denoise, mi355pt_denoise_var_device, then Sensor::to_rgb on the result as a film
// with spp 1.  Returns the device seconds of the two beauty launches.
static mi355pt_denoise_var_params denoise_var_params(float sigma_lum) {
    mi355pt_denoise_var_params dp;
    mi355pt_denoise_var_params_default(&dp);
    if (sigma_lum != 0.0f) dp.sigma_lum = sigma_lum;
    return dp;
}
static double render_denoised_variance(const Scene& scene, const Camera& camera, mi355pt_params p, uint32_t guide_spp, bool fused, float sigma_lum, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const uint32_t n_pixels = cam.width * cam.height;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), scratch_bytes = mi355pt_denoise_var_scratch_bytes(cam.width, cam.height);
    DeviceFilm beauty(film_bytes), half(film_bytes), albedo(film_bytes), normal(film_bytes), out(film_bytes), rgb(film_bytes), scratch(scratch_bytes);
    mi355pt_stats st0{}, st1{};
    check(mi355pt_render_accum_device(scene.raw(), &cam, &p, 0, p.spp / 2, half.p, nullptr, &st0), "mi355pt_render_accum_device");
    if (hipMemcpy(beauty.p, half.p, film_bytes, hipMemcpyDeviceToDevice) != hipSuccess) throw std::runtime_error("mi355pt: copying the half film failed");
    check(mi355pt_render_accum_device(scene.raw(), &cam, &p, p.spp / 2, p.spp, beauty.p, nullptr, &st1), "mi355pt_render_accum_device");
    render_guides(scene, cam, p, guide_spp, fused, albedo.p, normal.p);
    const mi355pt_denoise_var_params dp = denoise_var_params(sigma_lum);
    check(mi355pt_denoise_var_device(beauty.p, half.p, p.spp, nullptr, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp, scratch.p, scratch_bytes,
                                     out.p, nullptr), "mi355pt_denoise_var_device");
    display_stage.resolve(out.p, cam.width, cam.height, 1, rgb.p);
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    return (st0.kernel_ms + st1.kernel_ms) * 1e-3;
}

// --adaptive-threshold: mi355pt_render_adaptive_device with --spp as the maximum, the per-tile means (a film with spp 1), optionally the
// denoiser on them — or, with --denoise-variance, the driver's film, half film and tile counts straight into that filter, no normalise step
// before it —, then Sensor::to_rgb.  --spp-map writes the samples per tile as a grey picture, log2(tile_spp / min) / log2(max / min).
static void render_adaptive(const Scene& scene, const Camera& camera, mi355pt_params p, const Args& a, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const uint32_t n_pixels = cam.width * cam.height, tiles_x = (cam.width + 7) / 8, n_tiles = tiles_x * ((cam.height + 7) / 8);
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), tile_bytes = (size_t)n_tiles * 4, scratch_bytes = mi355pt_adaptive_scratch_bytes(cam.width, cam.height);
    DeviceFilm film(film_bytes), half(film_bytes), rgb(film_bytes), tile_spp(tile_bytes), tile_err(tile_bytes), list(tile_bytes), scratch(scratch_bytes);
    const mi355pt_adaptive_params ap{a.adaptive_threshold, a.adaptive_dark_eps, a.adaptive_min_spp};
    mi355pt_adaptive_result res{};
    check(mi355pt_render_adaptive_device(scene.raw(), &cam, &p, &ap, film.p, half.p, (uint32_t*)tile_spp.p, tile_err.p, (uint32_t*)list.p, scratch.p, scratch_bytes,
                                         nullptr, &res), "mi355pt_render_adaptive_device");
    if (a.denoise_variance) {
        const uint32_t guide_spp = a.denoise_guide_spp;
        const size_t dn_bytes = mi355pt_denoise_var_scratch_bytes(cam.width, cam.height);
        DeviceFilm albedo(film_bytes), normal(film_bytes), out(film_bytes), dn_scratch(dn_bytes);
        render_guides(scene, cam, p, guide_spp, a.fused_guides, albedo.p, normal.p);
        const mi355pt_denoise_var_params dp = denoise_var_params(a.denoise_sigma_lum);
        check(mi355pt_denoise_var_device(film.p, half.p, 0, (const uint32_t*)tile_spp.p, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp,
                                         dn_scratch.p, dn_bytes, out.p, nullptr), "mi355pt_denoise_var_device");
        display_stage.resolve(out.p, cam.width, cam.height, 1, rgb.p);
    } else if (a.denoise) {
        check(mi355pt_film_normalize_tiles_device(film.p, (const uint32_t*)tile_spp.p, cam.width, cam.height, half.p, nullptr), "mi355pt_film_normalize_tiles_device");
        const uint32_t guide_spp = a.denoise_guide_spp;
        const size_t dn_bytes = mi355pt_denoise_scratch_bytes(cam.width, cam.height);
        DeviceFilm albedo(film_bytes), normal(film_bytes), dn_scratch(dn_bytes);
        render_guides(scene, cam, p, guide_spp, a.fused_guides, albedo.p, normal.p);
        mi355pt_denoise_params dp;
        mi355pt_denoise_params_default(&dp);
        check(mi355pt_denoise_device(half.p, 1, albedo.p, guide_spp, normal.p, guide_spp, cam.width, cam.height, &dp, dn_scratch.p, dn_bytes, film.p, nullptr), "mi355pt_denoise_device");
        display_stage.resolve(film.p, cam.width, cam.height, 1, rgb.p);
    } else {
        check(mi355pt_film_normalize_tiles_device(film.p, (const uint32_t*)tile_spp.p, cam.width, cam.height, half.p, nullptr), "mi355pt_film_normalize_tiles_device");
        display_stage.resolve(half.p, cam.width, cam.height, 1, rgb.p);
    }
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    std::printf("(adaptive: %u passes, mean %.1f spp of at most %u, %u of %u tiles at the maximum)\n", res.passes, (double)res.total_samples / n_pixels, p.spp,
                res.tiles_at_max, n_tiles);
    if (!a.spp_map.empty()) {
        std::vector<uint32_t> spp(n_tiles);
        if (hipMemcpy(spp.data(), tile_spp.p, tile_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the tile counts back failed");
        const double span = std::log2((double)p.spp / ap.min_spp);
        std::vector<uint8_t> grey((size_t)n_pixels * 3);
        for (uint32_t y = 0; y < cam.height; ++y)
            for (uint32_t x = 0; x < cam.width; ++x) {
                const double g = span > 0.0 ? std::log2((double)spp[(y / 8) * tiles_x + x / 8] / ap.min_spp) / span : 0.0;
                const uint8_t v = (uint8_t)(g * 255.0);
                uint8_t* o = &grey[((size_t)y * cam.width + x) * 3];
                o[0] = o[1] = o[2] = v;
            }
        write_png_rgb8(a.spp_map, grey.data(), cam.width, cam.height);
    }
}

// --renderer position | depth: the G-buffer pass's position and hit films at --spp, coverage-normalised on the device
// (mi355pt_gbuffer_normalize_device): the mean render-space hit position over the samples that hit, or the mean distance along the unit ray
// replicated to RGB; 0 where no sample hit.  Float output: `pixels` goes to a PFM as it is.  Returns the device seconds of the launch.
static double render_gbuffer_float(const Scene& scene, const Camera& camera, mi355pt_params p, bool depth, std::vector<float>& pixels) {
    const mi355pt_camera& cam = camera.raw();
    const uint32_t n_pixels = cam.width * cam.height;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float);
    DeviceFilm position(depth ? sizeof(float) : film_bytes), hit(film_bytes), out(film_bytes);
    const mi355pt_gbuffer_films films{nullptr, nullptr, depth ? nullptr : position.p, hit.p};
    mi355pt_stats st{};
    check(mi355pt_render_gbuffer_accum_device(scene.raw(), &cam, &p, scene.d65_lut(), 0, p.spp, &films, nullptr, &st), "mi355pt_render_gbuffer_accum_device");
    check(mi355pt_gbuffer_normalize_device(depth ? hit.p : position.p, hit.p, n_pixels, out.p, nullptr), "mi355pt_gbuffer_normalize_device");
    if (hipMemcpy(pixels.data(), out.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    if (depth) for (uint32_t i = 0; i < n_pixels; ++i) pixels[3 * (size_t)i + 1] = pixels[3 * (size_t)i + 2] = pixels[3 * (size_t)i];
    return st.kernel_ms * 1e-3;
}

// --camera-move: the scene of the --temporal-frames loops at the next frame's camera position.  rebuild (the default): mi355pt_scene_build
// again.  rebase: mi355pt_scene_move_camera — the built scene re-based and refit on the device — and one line per frame on stderr
static void follow_camera(Scene& scene, const Camera& moved, const Args& a, uint32_t frame) {
    if (a.camera_move != "rebase" && !(a.flow && !a.camera_move_given)) { scene.build(moved); return; }      // (--flow moves in place unless told to rebuild)
    const mi355pt_move_result r = scene.move_camera(moved);
    std::fprintf(stderr, "camera move, frame %u: rebuilt=%u host_ms=%.3f device_ms=%.3f\n", frame, r.rebuilt, r.host_ms, r.device_ms);
}

// --light-step, --emitter-gain, --env-yaw-step: the frame's step once more on top of what the scene holds (mi355pt_scene_edit), at the camera
// the scene is at; --scene-edit rebuild then builds the edited description again.  One line per frame on stderr
static void step_scene_edits(Scene& scene, const Camera& at, const Args& a, uint32_t frame) {
    std::vector<mi355pt_material_edit> mats; std::vector<mi355pt_light_edit> lights; std::vector<mi355pt_env_edit> envs;
    for (const Args::EmitterGain& g : a.emitter_gains) {
        mi355pt_material_edit e{g.mat, scene.material_desc(g.mat)};
        e.desc.intensity *= g.gain;
        mats.push_back(e);
    }
    for (const Args::LightStep& st : a.light_steps) {
        mi355pt_light_edit e{st.id, scene.light_desc(st.id)};
        for (int i = 0; i < 3; ++i) e.desc.local_to_world[12 + i] += st.d[i];
        e.desc.intensity *= st.gain;
        lights.push_back(e);
    }
    std::vector<std::vector<float>> turned;
    if (a.env_yaw_given) {
        const double r = (double)a.env_yaw_step * 3.14159265358979323846 / 180.0;
        const float c = (float)std::cos(r), sn = (float)std::sin(r);
        const float ry[16] = {c, 0, -sn, 0, 0, 1, 0, 0, sn, 0, c, 0, 0, 0, 0, 1};      // column-major R_y
        for (uint32_t v = 0; v < scene.env_count(); ++v) {
            const float* m = scene.env_transform(v);
            std::vector<float> o(16, 0.0f);
            for (int col = 0; col < 4; ++col) for (int row = 0; row < 4; ++row) for (int k = 0; k < 4; ++k) o[4 * col + row] += ry[4 * k + row] * m[4 * col + k];
            turned.push_back(o);
        }
        for (uint32_t v = 0; v < scene.env_count(); ++v) envs.push_back(mi355pt_env_edit{v, scene.env_intensity(v), turned[v].data(), nullptr});
    }
    const mi355pt_edit_result r = scene.edit(at, mats, lights, envs);
    std::fprintf(stderr, "scene edit, frame %u: rebuilt=%u reason=%u launches=%u features=%u->%u host_ms=%.3f device_ms=%.3f\n", frame, r.rebuilt, r.reason, r.launches,
                 r.features_before, r.features_after, r.host_ms, r.device_ms);
    if (a.scene_edit != "inplace" && !r.rebuilt) scene.build(at);
}

// One frame of the accumulation on device buffers: the entry point of the carry (ids_cur == nullptr: none; a table of n_entries records, or
// else flow records) and of --temporal-rectify (rect != nullptr: its parameters, with the scratch).  The name check() gets is the entry
// point's that ran
struct TemporalCarryArgs { const uint32_t *ids_cur = nullptr, *ids_prev = nullptr; const mi355pt_motion_xform* table = nullptr; uint32_t n_entries = 0; const mi355pt_flow_pixel* flow = nullptr; };
static void temporal_accumulate(const mi355pt_temporal_frame& cur, uint32_t spp, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                                uint32_t height, const mi355pt_temporal_params& tp, const TemporalCarryArgs& carry, const mi355pt_temporal_rectify_params* rect,
                                void* scratch, size_t scratch_bytes, float* out_film, float* out_half, float* out_length) {
    const uint32_t *ic = carry.ids_cur, *ip = carry.ids_prev;
    if (carry.flow && rect)
        check(mi355pt_temporal_accumulate_rectified_flow_device(&cur, spp, prev, view, width, height, &tp, rect, scratch, scratch_bytes, ic, ip, carry.flow, out_film,
                                                                out_half, out_length, nullptr), "mi355pt_temporal_accumulate_rectified_flow_device");
    else if (carry.flow)
        check(mi355pt_temporal_accumulate_flow_device(&cur, spp, prev, view, width, height, &tp, ic, ip, carry.flow, out_film, out_half, out_length, nullptr),
              "mi355pt_temporal_accumulate_flow_device");
    else if (carry.table && rect)
        check(mi355pt_temporal_accumulate_rectified_motion_device(&cur, spp, prev, view, width, height, &tp, rect, scratch, scratch_bytes, ic, ip, carry.table,
                                                                  carry.n_entries, out_film, out_half, out_length, nullptr),
              "mi355pt_temporal_accumulate_rectified_motion_device");
    else if (carry.table)
        check(mi355pt_temporal_accumulate_motion_device(&cur, spp, prev, view, width, height, &tp, ic, ip, carry.table, carry.n_entries, out_film, out_half, out_length,
                                                        nullptr), "mi355pt_temporal_accumulate_motion_device");
    else if (rect)
        check(mi355pt_temporal_accumulate_rectified_device(&cur, spp, prev, view, width, height, &tp, rect, scratch, scratch_bytes, out_film, out_half, out_length,
                                                           nullptr), "mi355pt_temporal_accumulate_rectified_device");
    else
        check(mi355pt_temporal_accumulate_device(&cur, spp, prev, view, width, height, &tp, out_film, out_half, out_length, nullptr),
              "mi355pt_temporal_accumulate_device");
}

// --temporal-frames N [--camera-step dx,dy,dz]: N frames of --spp samples, frame k with seed + k and the camera at position + k * step (the
// scene follows as --camera-move says: built again, mi355pt_scene_build bakes the position in, or re-based on the device).  Per frame one G-buffer launch at --denoise-guide-spp
// (shading normal, position, hit — and albedo when --denoise-variance follows), the beauty film (and the half film with --denoise-variance),
// then mi355pt_temporal_accumulate_device (with --temporal-rectify: mi355pt_temporal_accumulate_rectified_device, radius and gamma from
// --temporal-rectify-radius / --temporal-rectify-gamma or the defaults) against the previous frame's accumulated films.  After the last frame optionally the
// variance-guided filter on the accumulated pair (spp 2), then Sensor::to_rgb.  Returns the device seconds of the beauty launches.
// With --instance-step (mi355pt_motion.h) the named instances take their step once more before every frame but the first
// (mi355pt_scene_move_instances), and each frame adds one ID pass, the motion table of the two frames' matrices and cameras, and the
// motion-aware twin of the accumulation with the previous frame's ids.
// With --temporal-budget (mi355pt_budget.h) the order per frame is: G-buffer, ids / flow records, the history probe, the budget driver (--spp
// is its base count, the sample sequence that of the maximum), the pair normalise, the accumulation the other flags select with spp = 2 (always
// with the half film: the driver renders the pair), the length credit; the seconds returned are then wall time around the driver.
static double render_temporal(Scene& scene, const Camera& camera, mi355pt_params p, const Args& a, std::vector<float>& pixels) {
    const mi355pt_camera base = camera.raw();
    const uint32_t n_pixels = base.width * base.height, guide_spp = a.denoise_guide_spp;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), len_bytes = (size_t)n_pixels * sizeof(float);
    const bool half = a.denoise_variance, moving = a.camera_step[0] != 0.0f || a.camera_step[1] != 0.0f || a.camera_step[2] != 0.0f;
    const bool budgeting = a.temporal_budget, pair = half || budgeting;      // the accumulation runs on a film pair
    const size_t opt = half ? film_bytes : sizeof(float), popt = pair ? film_bytes : sizeof(float);
    const mi355pt_budget_params bp{p.spp, a.temporal_budget_max_given ? a.temporal_budget_max_spp : 8u * p.spp, a.temporal_budget_target};
    const size_t n_tiles = (size_t)((base.width + 7u) / 8u) * ((base.height + 7u) / 8u);
    const size_t budget_scratch_bytes = budgeting ? mi355pt_adaptive_scratch_bytes(base.width, base.height) : sizeof(float);
    DeviceFilm tile_len(budgeting ? n_tiles * sizeof(float) : sizeof(float)), tile_spp(budgeting ? n_tiles * sizeof(uint32_t) : sizeof(float));
    DeviceFilm tile_list(budgeting ? n_tiles * sizeof(uint32_t) : sizeof(float)), budget_scratch(budget_scratch_bytes);
    // two sets that alternate: the frame's G-buffer films and its accumulated pair with the length film
    DeviceFilm normal0(film_bytes), normal1(film_bytes), position0(film_bytes), position1(film_bytes), hit0(film_bytes), hit1(film_bytes);
    DeviceFilm acc0(film_bytes), acc1(film_bytes), acch0(popt), acch1(popt), len0(len_bytes), len1(len_bytes);
    DeviceFilm beauty(film_bytes), bhalf(popt), albedo(opt), rgb(film_bytes);
    float *normal[2] = {normal0.p, normal1.p}, *position[2] = {position0.p, position1.p}, *hit[2] = {hit0.p, hit1.p};
    float *acc[2] = {acc0.p, acc1.p}, *acch[2] = {acch0.p, acch1.p}, *len[2] = {len0.p, len1.p};
    mi355pt_temporal_params tp;
    mi355pt_temporal_params_default(&tp);
    mi355pt_temporal_rectify_params rp;
    mi355pt_temporal_rectify_params_default(&rp);
    if (a.temporal_rectify_radius_given) rp.radius = a.temporal_rectify_radius;
    if (a.temporal_rectify_gamma_given) rp.gamma = a.temporal_rectify_gamma;
    const size_t rectify_bytes = a.temporal_rectify ? mi355pt_temporal_rectify_scratch_bytes(base.width, base.height) : sizeof(float);
    DeviceFilm rectify_scratch(rectify_bytes);
    // --instance-step (mi355pt_motion.h): the frame's ids in two sets that alternate like the G-buffer, the motion table, every instance's
    // local_to_world in this frame and in the one before
    const bool stepping = !a.instance_steps.empty();
    const uint32_t n_inst = scene.instance_count();
    DeviceFilm ids0(stepping ? len_bytes : sizeof(float)), ids1(stepping ? len_bytes : sizeof(float));
    DeviceFilm table(stepping ? ((size_t)n_inst + 1) * sizeof(mi355pt_motion_xform) : sizeof(float));
    uint32_t* ids[2] = {(uint32_t*)ids0.p, (uint32_t*)ids1.p};
    std::vector<float> l2w_prev(stepping ? 16 * (size_t)n_inst : 0);
    // --flow (mi355pt_flow.h): the frame's motion records, the ids in the two alternating sets above, and the ORIGINAL vertices of the meshes
    // under --mesh-wave, which frame k deforms with phase k * phase_step
    const bool flowing = a.flow;
    DeviceFilm flow_ids0(flowing && !stepping ? len_bytes : sizeof(float)), flow_ids1(flowing && !stepping ? len_bytes : sizeof(float));
    if (flowing && !stepping) { ids[0] = (uint32_t*)flow_ids0.p; ids[1] = (uint32_t*)flow_ids1.p; }
    DeviceFilm flow_records(flowing ? (size_t)n_pixels * sizeof(mi355pt_flow_pixel) : sizeof(float));
    std::vector<std::vector<float>> wave_home;
    for (const Args::MeshWave& w : a.mesh_waves) wave_home.push_back(scene.mesh(w.geom).pos);
    mi355pt_camera cam = base, cam_prev = base;
    double kernel_ms = 0.0;
    for (uint32_t k = 0; k < a.temporal_frames; ++k) {
        const int c = (int)(k & 1u), q = c ^ 1;
        cam_prev = cam;
        for (int i = 0; i < 3; ++i) cam.position[i] = base.position[i] + (float)k * a.camera_step[i];
        Camera moved(base.fov_deg, base.width, base.height);
        moved.set_look_to({cam.position[0], cam.position[1], cam.position[2]}, {cam.direction[0], cam.direction[1], cam.direction[2]}, {cam.up[0], cam.up[1], cam.up[2]});
        if (flowing && k > 0) scene.flow_mark();      // the positions of frame k - 1, ahead of every move of frame k
        if (k > 0 && moving) follow_camera(scene, moved, a, k);
        for (uint32_t i = 0; stepping && i < n_inst; ++i) std::memcpy(&l2w_prev[16 * (size_t)i], scene.instance_transform(i), 16 * sizeof(float));
        if (k > 0 && stepping) {      // the step once more on top of the last frame's matrix, at the camera the scene is at now
            std::vector<uint32_t> step_ids; std::vector<float> matrices(16 * a.instance_steps.size());
            for (size_t j = 0; j < a.instance_steps.size(); ++j) {
                step_ids.push_back(a.instance_steps[j].id);
                instance_transform_matrix(a.instance_steps[j], scene.instance_transform(step_ids.back()), &matrices[16 * j]);
            }
            const mi355pt_instance_move_result mr = scene.move_instances(moved, step_ids, matrices);
            std::fprintf(stderr, "instance step, frame %u: rebuilt=%u reason=%u host_ms=%.3f device_ms=%.3f\n", k, mr.rebuilt, mr.reason, mr.host_ms, mr.device_ms);
        }
        if (flowing && !a.mesh_waves.empty()) {      // frame k's wave on the original vertices (frame 0: phase 0)
            std::vector<uint32_t> geoms; std::vector<std::vector<float>> pos, nrm;
            for (size_t j = 0; j < a.mesh_waves.size(); ++j) {
                geoms.push_back(a.mesh_waves[j].geom);
                pos.push_back(waved_positions(a.mesh_waves[j], wave_home[j], (double)k * (double)a.mesh_waves[j].phase_step));
                nrm.push_back(area_weighted_normals(scene.mesh(geoms.back()), pos.back()));
            }
            const mi355pt_instance_move_result mr = scene.deform_meshes(moved, geoms, pos, nrm, a.instance_rebuild_above);
            std::fprintf(stderr, "mesh deform, frame %u: rebuilt=%u reason=%u host_ms=%.3f device_ms=%.3f\n", k, mr.rebuilt, mr.reason, mr.host_ms, mr.device_ms);
        }
        if (k > 0 && a.editing()) step_scene_edits(scene, moved, a, k);
        // a move that built the scene again dropped the mark: this frame has no previous one
        const bool first = k == 0 || (flowing && !scene.flow_marked());
        if (flowing && k > 0 && first) std::fprintf(stderr, "flow, frame %u: a move rebuilt the scene, the accumulation restarts\n", k);
        p.seed = a.seed + k;
        bool ok = hipMemset(normal[c], 0, film_bytes) == hipSuccess && hipMemset(position[c], 0, film_bytes) == hipSuccess && hipMemset(hit[c], 0, film_bytes) == hipSuccess &&
                  hipMemset(beauty.p, 0, film_bytes) == hipSuccess;
        if (half) ok = ok && hipMemset(bhalf.p, 0, film_bytes) == hipSuccess && hipMemset(albedo.p, 0, film_bytes) == hipSuccess;
        if (budgeting && !half) ok = ok && hipMemset(bhalf.p, 0, film_bytes) == hipSuccess;
        if (!ok) throw std::runtime_error("mi355pt: clearing the frame's films failed");
        mi355pt_params g = p;
        g.spp = guide_spp;
        const mi355pt_gbuffer_films films{half ? albedo.p : nullptr, normal[c], position[c], hit[c]};
        check(mi355pt_render_gbuffer_accum_device(scene.raw(), &cam, &g, scene.d65_lut(), 0, guide_spp, &films, nullptr, nullptr), "mi355pt_render_gbuffer_accum_device");
        const mi355pt_temporal_frame cur{beauty.p, pair ? bhalf.p : nullptr, nullptr, position[c], normal[c], hit[c]};
        const mi355pt_temporal_frame prev{acc[q], pair ? acch[q] : nullptr, len[q], position[q], normal[q], hit[q]};
        mi355pt_temporal_view view{};
        if (k > 0) check(mi355pt_temporal_view_from_cameras(&cam, &cam_prev, &view), "mi355pt_temporal_view_from_cameras");
        // how the frame's pixels are carried one frame back (no launch of it depends on the beauty film, which follows)
        TemporalCarryArgs carry;
        if (flowing) {                // the flow pass against the mark (a first frame: the ids alone), the flow-aware accumulation with the previous ids
            carry.flow = (mi355pt_flow_pixel*)flow_records.p;
            if (first) scene.ids_device(cam, g, ids[c]); else scene.flow_device(cam, g, (mi355pt_flow_pixel*)flow_records.p, ids[c]);
        } else if (stepping) {        // one ID pass, the table of the two frames' matrices and cameras, the motion-aware accumulation with the previous ids
            scene.ids_device(cam, g, ids[c]);
            const std::vector<mi355pt_motion_xform> host_table = scene.motion_table(cam, cam_prev, l2w_prev);
            if (hipMemcpy(table.p, host_table.data(), host_table.size() * sizeof(mi355pt_motion_xform), hipMemcpyHostToDevice) != hipSuccess)
                throw std::runtime_error("mi355pt: copying the motion table failed");
            carry.table = (const mi355pt_motion_xform*)table.p; carry.n_entries = n_inst + 1;
        }
        const bool has_prev = flowing ? !first : k > 0;
        if (flowing || stepping) { carry.ids_cur = ids[c]; carry.ids_prev = has_prev ? ids[q] : nullptr; }
        uint32_t frame_spp = p.spp;
        if (budgeting) {              // probe, driver, pair normalise: the frame becomes a film pair with spp = 2
            const mi355pt_budget_motion motion{carry.ids_cur, carry.ids_prev, carry.table, carry.n_entries, carry.flow};
            check(mi355pt_temporal_budget_device(&cur, has_prev ? &prev : nullptr, has_prev ? &view : nullptr, base.width, base.height, &tp, &motion, &bp, nullptr,
                                                 tile_len.p, (uint32_t*)tile_spp.p, nullptr), "mi355pt_temporal_budget_device");
            mi355pt_params pb = p;
            pb.spp = bp.max_spp;
            mi355pt_adaptive_result res{};
            if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("mi355pt: waiting for the history probe failed");
            const auto t0 = std::chrono::steady_clock::now();
            check(mi355pt_render_budget_device(scene.raw(), &cam, &pb, &bp, (const uint32_t*)tile_spp.p, beauty.p, bhalf.p, (uint32_t*)tile_list.p, budget_scratch.p,
                                               budget_scratch_bytes, nullptr, &res), "mi355pt_render_budget_device");
            if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("mi355pt: waiting for the budget driver failed");
            kernel_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "temporal budget, frame %u: passes=%u tiles_at_max=%u total_samples=%llu (uniform %u spp: %llu)\n", k, res.passes, res.tiles_at_max,
                         (unsigned long long)res.total_samples, p.spp, (unsigned long long)p.spp * n_pixels);
            check(mi355pt_film_pair_normalize_tiles_device(beauty.p, bhalf.p, (const uint32_t*)tile_spp.p, base.width, base.height, beauty.p, bhalf.p, nullptr),
                  "mi355pt_film_pair_normalize_tiles_device");
            frame_spp = 2;
        } else {
            mi355pt_stats st0{}, st1{};
            if (half) {
                check(mi355pt_render_accum_device(scene.raw(), &cam, &p, 0, p.spp / 2, bhalf.p, nullptr, &st0), "mi355pt_render_accum_device");
                if (hipMemcpy(beauty.p, bhalf.p, film_bytes, hipMemcpyDeviceToDevice) != hipSuccess) throw std::runtime_error("mi355pt: copying the half film failed");
                check(mi355pt_render_accum_device(scene.raw(), &cam, &p, p.spp / 2, p.spp, beauty.p, nullptr, &st1), "mi355pt_render_accum_device");
            } else {
                check(mi355pt_render_accum_device(scene.raw(), &cam, &p, 0, p.spp, beauty.p, nullptr, &st0), "mi355pt_render_accum_device");
            }
            kernel_ms += st0.kernel_ms + st1.kernel_ms;
        }
        temporal_accumulate(cur, frame_spp, has_prev ? &prev : nullptr, has_prev ? &view : nullptr, base.width, base.height, tp, carry, a.temporal_rectify ? &rp : nullptr,
                            rectify_scratch.p, rectify_bytes, acc[c], pair ? acch[c] : nullptr, len[c]);
        if (budgeting)
            check(mi355pt_temporal_length_credit_device(len[c], (const uint32_t*)tile_spp.p, bp.base_spp, tp.max_history, base.width, base.height, nullptr),
                  "mi355pt_temporal_length_credit_device");
        display_stage.meter(acc[c], base.width, base.height, pair ? 2u : 1u);      // --auto-exposure: every frame, with the previous frame's record
    }
    const int last = (int)((a.temporal_frames - 1) & 1u);
    if (half) {
        const size_t scratch_bytes = mi355pt_denoise_var_scratch_bytes(base.width, base.height);
        DeviceFilm out(film_bytes), scratch(scratch_bytes);
        const mi355pt_denoise_var_params dp = denoise_var_params(a.denoise_sigma_lum);
        check(mi355pt_denoise_var_device(acc[last], acch[last], 2, nullptr, albedo.p, guide_spp, normal[last], guide_spp, base.width, base.height, &dp, scratch.p,
                                         scratch_bytes, out.p, nullptr), "mi355pt_denoise_var_device");
        display_stage.resolve(out.p, base.width, base.height, 1, rgb.p);
        if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    } else {
        display_stage.resolve(acc[last], base.width, base.height, pair ? 2u : 1u, rgb.p);      // (--temporal-budget alone: a pair, spp 2)
        if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    }
    return kernel_ms * 1e-3;
}

// --half-res [--half-res-albedo]: the paths are traced at width / 2 x height / 2 and the frame is rebuilt at width x height
// (mi355pt_upsample.h).  Per frame: the camera of the low frame from mi355pt_upsample_low_camera, rendered on the SAME built scene (a build
// fixes the position only); the low and the full G-buffer at --denoise-guide-spp (shading normal, position, hit — the low albedo with
// --half-res-albedo, the full albedo with it or when --denoise-variance follows); the low beauty film (and the low half film with
// --denoise-variance); mi355pt_upsample_device.  With --temporal-frames N the upsampled pair is the current frame (spp 2, or 1 without a half
// film) of the accumulation of render_temporal, frame k with seed + k from position + k * step.  Then optionally the variance-guided filter on
// the pair (spp 2) with the full guides, then Sensor::to_rgb.  Returns the device seconds of the (low) beauty launches.
static double render_half_res(Scene& scene, const Camera& camera, mi355pt_params p, const Args& a, std::vector<float>& pixels) {
    const mi355pt_camera base = camera.raw();
    const uint32_t n_pixels = base.width * base.height, n_low = (base.width / 2) * (base.height / 2), guide_spp = a.denoise_guide_spp;
    const size_t film_bytes = (size_t)n_pixels * 3 * sizeof(float), low_bytes = (size_t)n_low * 3 * sizeof(float), len_bytes = (size_t)n_pixels * sizeof(float);
    const bool half = a.denoise_variance, demod = a.half_res_albedo, full_albedo = demod || half;
    const bool moving = a.camera_step[0] != 0.0f || a.camera_step[1] != 0.0f || a.camera_step[2] != 0.0f;
    const uint32_t frames = a.temporal ? a.temporal_frames : 1u, up_spp = half ? 2u : 1u;
    const size_t opt = half ? film_bytes : sizeof(float), topt = a.temporal ? film_bytes : sizeof(float), thopt = a.temporal && half ? film_bytes : sizeof(float);
    // the full G-buffer in two sets that alternate (the temporal accumulation reads the previous frame's), the low one, the low films, the upsampled pair
    DeviceFilm normal0(film_bytes), normal1(topt), position0(film_bytes), position1(topt), hit0(film_bytes), hit1(topt), albedo(full_albedo ? film_bytes : sizeof(float));
    DeviceFilm lnormal(low_bytes), lposition(low_bytes), lhit(low_bytes), lalbedo(demod ? low_bytes : sizeof(float)), lbeauty(low_bytes), lhalf(half ? low_bytes : sizeof(float));
    DeviceFilm up(film_bytes), uph(opt), rgb(film_bytes);
    DeviceFilm acc0(topt), acc1(topt), acch0(thopt), acch1(thopt), len0(a.temporal ? len_bytes : sizeof(float)), len1(a.temporal ? len_bytes : sizeof(float));
    float *normal[2] = {normal0.p, a.temporal ? normal1.p : normal0.p}, *position[2] = {position0.p, a.temporal ? position1.p : position0.p};
    float *hit[2] = {hit0.p, a.temporal ? hit1.p : hit0.p}, *acc[2] = {acc0.p, acc1.p}, *acch[2] = {acch0.p, acch1.p}, *len[2] = {len0.p, len1.p};
    mi355pt_upsample_params up_params;
    mi355pt_upsample_params_default(&up_params);
    mi355pt_temporal_params tp;
    mi355pt_temporal_params_default(&tp);
    mi355pt_temporal_rectify_params rp;
    mi355pt_temporal_rectify_params_default(&rp);
    if (a.temporal_rectify_radius_given) rp.radius = a.temporal_rectify_radius;
    if (a.temporal_rectify_gamma_given) rp.gamma = a.temporal_rectify_gamma;
    const size_t rectify_bytes = a.temporal_rectify ? mi355pt_temporal_rectify_scratch_bytes(base.width, base.height) : sizeof(float);
    DeviceFilm rectify_scratch(rectify_bytes);
    mi355pt_camera cam = base, cam_prev = base, low_cam{};
    double kernel_ms = 0.0;
    int c = 0;
    for (uint32_t k = 0; k < frames; ++k) {
        c = (int)(k & 1u);
        const int q = c ^ 1;
        cam_prev = cam;
        for (int i = 0; i < 3; ++i) cam.position[i] = base.position[i] + (float)k * a.camera_step[i];
        if (k > 0 && moving) {
            Camera moved(base.fov_deg, base.width, base.height);
            moved.set_look_to({cam.position[0], cam.position[1], cam.position[2]}, {cam.direction[0], cam.direction[1], cam.direction[2]}, {cam.up[0], cam.up[1], cam.up[2]});
            follow_camera(scene, moved, a, k);
        }
        check(mi355pt_upsample_low_camera(&cam, &low_cam), "mi355pt_upsample_low_camera");
        p.seed = a.seed + k;
        bool ok = hipMemset(normal[c], 0, film_bytes) == hipSuccess && hipMemset(position[c], 0, film_bytes) == hipSuccess && hipMemset(hit[c], 0, film_bytes) == hipSuccess &&
                  hipMemset(lnormal.p, 0, low_bytes) == hipSuccess && hipMemset(lposition.p, 0, low_bytes) == hipSuccess && hipMemset(lhit.p, 0, low_bytes) == hipSuccess &&
                  hipMemset(lbeauty.p, 0, low_bytes) == hipSuccess;
        if (full_albedo) ok = ok && hipMemset(albedo.p, 0, film_bytes) == hipSuccess;
        if (demod) ok = ok && hipMemset(lalbedo.p, 0, low_bytes) == hipSuccess;
        if (half) ok = ok && hipMemset(lhalf.p, 0, low_bytes) == hipSuccess;
        if (!ok) throw std::runtime_error("mi355pt: clearing the frame's films failed");
        mi355pt_params g = p;
        g.spp = guide_spp;
        const mi355pt_gbuffer_films full_films{full_albedo ? albedo.p : nullptr, normal[c], position[c], hit[c]};
        const mi355pt_gbuffer_films low_films{demod ? lalbedo.p : nullptr, lnormal.p, lposition.p, lhit.p};
        check(mi355pt_render_gbuffer_accum_device(scene.raw(), &cam, &g, scene.d65_lut(), 0, guide_spp, &full_films, nullptr, nullptr), "mi355pt_render_gbuffer_accum_device");
        check(mi355pt_render_gbuffer_accum_device(scene.raw(), &low_cam, &g, scene.d65_lut(), 0, guide_spp, &low_films, nullptr, nullptr), "mi355pt_render_gbuffer_accum_device");
        mi355pt_stats st0{}, st1{};
        if (half) {
            check(mi355pt_render_accum_device(scene.raw(), &low_cam, &p, 0, p.spp / 2, lhalf.p, nullptr, &st0), "mi355pt_render_accum_device");
            if (hipMemcpy(lbeauty.p, lhalf.p, low_bytes, hipMemcpyDeviceToDevice) != hipSuccess) throw std::runtime_error("mi355pt: copying the half film failed");
            check(mi355pt_render_accum_device(scene.raw(), &low_cam, &p, p.spp / 2, p.spp, lbeauty.p, nullptr, &st1), "mi355pt_render_accum_device");
        } else {
            check(mi355pt_render_accum_device(scene.raw(), &low_cam, &p, 0, p.spp, lbeauty.p, nullptr, &st0), "mi355pt_render_accum_device");
        }
        kernel_ms += st0.kernel_ms + st1.kernel_ms;
        const mi355pt_upsample_guides lg{demod ? lalbedo.p : nullptr, lnormal.p, lposition.p, lhit.p};
        const mi355pt_upsample_guides fg{demod ? albedo.p : nullptr, normal[c], position[c], hit[c]};
        check(mi355pt_upsample_device(lbeauty.p, half ? lhalf.p : nullptr, p.spp, &lg, guide_spp, &fg, guide_spp, base.width, base.height, &up_params, up.p,
                                      half ? uph.p : nullptr, nullptr), "mi355pt_upsample_device");
        if (!a.temporal) continue;
        const mi355pt_temporal_frame cur{up.p, half ? uph.p : nullptr, nullptr, position[c], normal[c], hit[c]};
        const mi355pt_temporal_frame prev{acc[q], half ? acch[q] : nullptr, len[q], position[q], normal[q], hit[q]};
        mi355pt_temporal_view view{};
        if (k > 0) check(mi355pt_temporal_view_from_cameras(&cam, &cam_prev, &view), "mi355pt_temporal_view_from_cameras");
        temporal_accumulate(cur, up_spp, k > 0 ? &prev : nullptr, k > 0 ? &view : nullptr, base.width, base.height, tp, TemporalCarryArgs{},
                            a.temporal_rectify ? &rp : nullptr, rectify_scratch.p, rectify_bytes, acc[c], half ? acch[c] : nullptr, len[c]);
        display_stage.meter(acc[c], base.width, base.height, up_spp);      // --auto-exposure: every frame, with the previous frame's record
    }
    const float* film = a.temporal ? acc[c] : up.p;           // the pair that leaves the loop: spp 2 with a half film; a mean without (the accumulation's, the upsample's)
    const float* film_half = a.temporal ? acch[c] : uph.p;
    if (half) {
        const size_t scratch_bytes = mi355pt_denoise_var_scratch_bytes(base.width, base.height);
        DeviceFilm out(film_bytes), scratch(scratch_bytes);
        const mi355pt_denoise_var_params dp = denoise_var_params(a.denoise_sigma_lum);
        check(mi355pt_denoise_var_device(film, film_half, 2, nullptr, albedo.p, guide_spp, normal[c], guide_spp, base.width, base.height, &dp, scratch.p, scratch_bytes,
                                         out.p, nullptr), "mi355pt_denoise_var_device");
        display_stage.resolve(out.p, base.width, base.height, 1, rgb.p);
    } else {
        display_stage.resolve(film, base.width, base.height, 1, rgb.p);
    }
    if (hipMemcpy(pixels.data(), rgb.p, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("mi355pt: copying the frame back failed");
    return kernel_ms * 1e-3;
}

static void usage() {
    std::puts("Usage: mi355pt [--scene N] [-s|--spp N] [--seed N] [--filter box] [--sampler random|sobol]\n"
              "               [--renderer normal|albedo|pt|nee|mis] [--width N] [--height N] [-d|--max-depth N] [-o|--output FILE]\n"
              "       extensions: [--albedo-lut] (clearcoat albedo from its table instead of the 64-sample estimate)  [--gpus N]\n"
              "                   [--renderer shading-normal] (render-space shading normal of every surface: the AOV a denoiser takes)\n"
              "                   [--denoise] (pt|nee|mis: a-trous filter guided by the albedo and shading-normal films)  [--denoise-guide-spp N] (64)\n"
              "                   [--denoise-variance] (pt|nee|mis, instead of --denoise: a-trous filter whose edge stop follows the variance that the film and a half\n"
              "                                         film give; --spp even; with --adaptive-threshold it takes the driver's films)  [--denoise-sigma-lum X] (4)\n"
              "                   [--adaptive-threshold X] (pt|nee|mis: samples where the per-tile noise estimate is above X; --spp is the maximum)\n"
              "                   [--adaptive-min-spp N] (16)  [--adaptive-dark-eps E] (1e-3)  [--spp-map FILE] (samples per tile as a grey picture)\n"
              "                   [--renderer position|depth] (the G-buffer pass: mean render-space hit position / mean distance over the samples that hit,\n"
              "                                                0 where none did; float output, -o must end in .pfm)\n"
              "                   [--fused-guides] (with --denoise or --denoise-variance: both guide films from one G-buffer launch, the same primary rays)\n"
              "                   [--temporal-frames N] (pt|nee|mis: N frames of --spp samples, frame k with seed + k, each reprojected into the next through its\n"
              "                                          G-buffer at --denoise-guide-spp and accumulated; writes the last; --denoise-variance filters the accumulated pair)\n"
              "                   [--camera-step dx,dy,dz] (with --temporal-frames: frame k renders from position + k * step)\n"
              "                   [--camera-move rebuild|rebase] (with --temporal-frames: between frames the scene is built again (the default) or the built\n"
              "                                 scene follows the camera on the device, mi355pt_scene_move_camera; one line per frame on stderr)\n"
              "                   [--temporal-rectify] (with --temporal-frames: the gathered history is first scaled so that its local mean agrees with the\n"
              "                                         current frame's: the accumulation follows a change of illumination)\n"
              "                   [--temporal-rectify-radius R] (2; 1 .. 3: the window is (2R + 1)^2 pixels)  [--temporal-rectify-gamma G] (2; > 0: standard errors allowed)\n"
              "                   [--half-res] (pt|nee|mis, even --width and --height: the paths are traced at half the width and height and the frame is rebuilt at\n"
              "                                 full size through the G-buffers of both sizes at --denoise-guide-spp; with --denoise-variance and --temporal-frames)\n"
              "                   [--half-res-albedo] (with --half-res: the low film is divided by the low albedo and multiplied by the full one)\n"
              "                   [--tone-map none|reinhard|reinhard-ext|aces|hable] (pt|nee|mis: the display stage's curve instead of the resolve's Reinhard)\n"
              "                   [--white W] (11.2; with --tone-map reinhard-ext|hable: the luminance / value that maps to 1)\n"
              "                   [--auto-exposure] (pt|nee|mis: the exposure from the frame's trimmed luminance histogram; with --temporal-frames every\n"
              "                                      frame is metered and blended with the previous frame's exposure)\n"
              "                   [--exposure-key K] (0.18: the value the mean luminance is mapped to)  [--exposure-adapt A] (1; 0 .. 1: the share of the way\n"
              "                                      to the new exposure taken per frame)  [--exposure-trim LO,HI] (102,51: 1/1024ths of the pixels left out)\n"
              "                   [--bloom] (pt|nee|mis: glare between the exposure and the tone curve of every path that ends on the device — a bright pass,\n"
              "                              a pyramid of blurs, a composite with the frame, mi355pt_bloom_device; metered before, never fed back into --temporal-frames)\n"
              "                   [--bloom-levels L] (6; 1 .. 8)  [--bloom-threshold T] (0; exposed units)  [--bloom-knee K] (0.5; 0 .. 1)  [--bloom-scatter S] (0.7; 0 .. 1)\n"
              "                   [--bloom-intensity I] (0.04; the frame keeps 1 - I)  [--bloom-additive] (the frame keeps 1, I up to 16, T 1 unless given)\n"
              "                   [--bloom-no-firefly] (no luminance weights in the first reduction)\n"
              "                   [--robust-buckets K] (pt|nee|mis, K = 4|8|16|32 dividing --spp: the frame as K buckets of consecutive samples, combined per\n"
              "                                         pixel by a trimmed mean of the bucket means: firefly rejection; with --denoise, --denoise-variance,\n"
              "                                         --fused-guides, --tone-map and --auto-exposure)\n"
              "                   [--robust-mode gmon|mom|mean] (gmon: the trim follows the Gini coefficient of the bucket means; mom: the median of means;\n"
              "                                         mean: no trim)  [--robust-scale X] (1; >= 0: the factor on the Gini term)\n"
              "                   [--instance-transform ID:tx,ty,tz[:ry_deg[:sx,sy,sz]]] (repeatable; pt|nee|mis|normal|albedo|position|depth: the scene is\n"
              "                                         built as described with instance ID marked dynamic, then its local_to_world becomes\n"
              "                                         T . R_y . S . local_to_world on the device, mi355pt_scene_move_instances; one line on stderr.\n"
              "                                         Not with --temporal-frames: a pose set once before the frame has no motion; --instance-step moves\n"
              "                                         instances across the frames with the object motion vectors of mi355pt_motion.h)\n"
              "                   [--instance-step ID:tx,ty,tz[:ry_deg]] (repeatable, distinct IDs; with --temporal-frames: in frame k the instance's local_to_world\n"
              "                                         is the scene's with T . R_y applied k times; the instances are moved on the device between the frames,\n"
              "                                         and each frame adds an ID pass, a motion table and the motion-aware accumulation.  Not with --half-res)\n"
              "                   [--instance-rebuild-above X] (0 = never; with --instance-transform: build again when the refit tree's SAH cost exceeds X\n"
              "                                         times the built tree's; applies to --mesh-wave too)\n"
              "                   [--temporal-budget TARGET] (with --temporal-frames: every frame probes the history length its pixels will find, renders --spp\n"
              "                                         samples everywhere and doubles them, up to --temporal-budget-max-spp, on the 8 x 8 tiles that would not reach\n"
              "                                         TARGET frames' worth; --spp a power of two; not with --half-res)  [--temporal-budget-max-spp M] (8 x --spp)\n"
              "                   [--light-step ID:dx,dy,dz[:gain]] [--emitter-gain MAT:g] [--env-yaw-step DEG] (repeatable but for the last; with --temporal-frames:\n"
              "                                         before every frame but the first delta light ID moves by (dx,dy,dz) and its intensity is multiplied by gain, the\n"
              "                                         emissive material MAT's intensity by g, every environment light turns by DEG degrees about +y)\n"
              "                   [--scene-edit inplace|rebuild] (how those steps reach the built scene: mi355pt_scene_edit in place, or the edited description built\n"
              "                                         again (the default).  Without --temporal-rectify the plain accumulation averages the change over its history)\n"
              "                   [--flow] (with --temporal-frames: per-pixel motion vectors — every frame marks the scene, takes --camera-step, --instance-step and\n"
              "                                         --mesh-wave in place (frame k's wave: the original vertices at phase k * phase_step) and accumulates through\n"
              "                                         the flow pass; a move that rebuilds restarts the accumulation; the camera follows as with --camera-move rebase unless\n"
              "                                         --camera-move rebuild is given.  Not with --half-res)\n"
              "                   [--mesh-wave GEOM:amp,wavelength[,phase_step]] (repeatable, distinct GEOMs; pt|nee|mis|normal|albedo|position|depth: the scene is\n"
              "                                         built as described, then every vertex of mesh GEOM takes y += amp sin(2 pi x / wavelength + phase_step)\n"
              "                                         in local space, with area-weighted vertex normals, on the device: mi355pt_scene_deform_meshes; one line\n"
              "                                         on stderr.  With --temporal-frames only under --flow: the other reprojections assume a static world\n"
              "                                         or rigid motion per instance)");
}

int main(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) { usage(); std::exit(2); } return argv[++i]; };
        if (k == "--scene") a.scene = (uint32_t)std::stoul(val());
        else if (k == "-s" || k == "--spp") a.spp = (uint32_t)std::stoul(val());
        else if (k == "--seed") a.seed = (uint32_t)std::stoul(val());
        else if (k == "--filter") a.filter = val();
        else if (k == "--sampler") a.sampler = val();
        else if (k == "--renderer") a.renderer = val();
        else if (k == "--width") a.width = (uint32_t)std::stoul(val());
        else if (k == "--height") a.height = (uint32_t)std::stoul(val());
        else if (k == "-d" || k == "--max-depth") a.max_depth = (uint32_t)std::stoul(val());
        else if (k == "-o" || k == "--output") a.output = val();
        else if (k == "--albedo-lut") a.albedo_lut = true;
        else if (k == "--gpus") a.gpus = std::stoi(val());
        else if (k == "--denoise") a.denoise = true;
        else if (k == "--denoise-variance") a.denoise_variance = true;
        else if (k == "--denoise-sigma-lum") a.denoise_sigma_lum = std::stof(val());
        else if (k == "--denoise-guide-spp") a.denoise_guide_spp = (uint32_t)std::stoul(val());
        else if (k == "--adaptive-threshold") a.adaptive_threshold = std::stof(val());
        else if (k == "--adaptive-min-spp") a.adaptive_min_spp = (uint32_t)std::stoul(val());
        else if (k == "--adaptive-dark-eps") a.adaptive_dark_eps = std::stof(val());
        else if (k == "--spp-map") a.spp_map = val();
        else if (k == "--fused-guides") a.fused_guides = true;
        else if (k == "--temporal-frames") { a.temporal = true; a.temporal_frames = (uint32_t)std::stoul(val()); }
        else if (k == "--temporal-rectify") a.temporal_rectify = true;
        else if (k == "--temporal-rectify-radius") { a.temporal_rectify_radius_given = true; a.temporal_rectify_radius = (uint32_t)std::stoul(val()); }
        else if (k == "--temporal-rectify-gamma") { a.temporal_rectify_gamma_given = true; a.temporal_rectify_gamma = std::stof(val()); }
        else if (k == "--half-res") a.half_res = true;
        else if (k == "--flow") a.flow = true;
        else if (k == "--temporal-budget") { a.temporal_budget = true; a.temporal_budget_target = std::stof(val()); }
        else if (k == "--temporal-budget-max-spp") { a.temporal_budget_max_given = true; a.temporal_budget_max_spp = (uint32_t)std::stoul(val()); }
        else if (k == "--half-res-albedo") a.half_res_albedo = true;
        else if (k == "--tone-map") a.tone_map = val();
        else if (k == "--white") { a.white_given = true; a.white = std::stof(val()); }
        else if (k == "--auto-exposure") a.auto_exposure = true;
        else if (k == "--exposure-key") { a.exposure_key_given = true; a.exposure_key = std::stof(val()); }
        else if (k == "--exposure-adapt") { a.exposure_adapt_given = true; a.exposure_adapt = std::stof(val()); }
        else if (k == "--exposure-trim") {
            const std::string v = val();
            char tail = 0;
            a.exposure_trim_given = true;
            if (std::sscanf(v.c_str(), "%u,%u%c", &a.exposure_trim[0], &a.exposure_trim[1], &tail) != 2 || (uint64_t)a.exposure_trim[0] + a.exposure_trim[1] >= 1024u) {
                std::fprintf(stderr, "error: invalid value '%s' for '--exposure-trim': two counts of 1/1024ths LO,HI whose sum is below 1024\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--bloom") a.bloom = true;
        else if (k == "--bloom-additive") a.bloom_additive = true;
        else if (k == "--bloom-no-firefly") a.bloom_no_firefly = true;
        else if (k == "--bloom-levels") {
            const std::string v = val();
            char tail = 0;
            a.bloom_levels_given = true;
            if (std::sscanf(v.c_str(), "%u%c", &a.bloom_levels, &tail) != 1 || a.bloom_levels < 1u || a.bloom_levels > MI355PT_BLOOM_MAX_LEVELS) {
                std::fprintf(stderr, "error: invalid value '%s' for '--bloom-levels': 1 .. 8\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--bloom-threshold" || k == "--bloom-knee" || k == "--bloom-scatter" || k == "--bloom-intensity") {
            const std::string v = val();
            char tail = 0;
            float x = 0.0f;
            const bool parsed = std::sscanf(v.c_str(), "%f%c", &x, &tail) == 1;
            const float hi = k == "--bloom-threshold" ? 0x1p16f : (k == "--bloom-intensity" ? 16.0f : 1.0f);
            if (!parsed || !(x >= 0.0f && x <= hi)) { std::fprintf(stderr, "error: invalid value '%s' for '%s': a number in [0, %g]\n", v.c_str(), k.c_str(), (double)hi); return 2; }
            if (k == "--bloom-threshold") { a.bloom_threshold_given = true; a.bloom_threshold = x; }
            else if (k == "--bloom-knee") { a.bloom_knee_given = true; a.bloom_knee = x; }
            else if (k == "--bloom-scatter") { a.bloom_scatter_given = true; a.bloom_scatter = x; }
            else { a.bloom_intensity_given = true; a.bloom_intensity = x; }
        }
        else if (k == "--robust-buckets") { a.robust_given = true; a.robust_buckets = (uint32_t)std::stoul(val()); }
        else if (k == "--robust-mode") a.robust_mode = val();
        else if (k == "--robust-scale") { a.robust_scale_given = true; a.robust_scale = std::stof(val()); }
        else if (k == "--camera-step") {
            const std::string v = val();
            char tail = 0;
            a.camera_step_given = true;
            if (std::sscanf(v.c_str(), "%f,%f,%f%c", &a.camera_step[0], &a.camera_step[1], &a.camera_step[2], &tail) != 3 || !std::isfinite(a.camera_step[0]) ||
                !std::isfinite(a.camera_step[1]) || !std::isfinite(a.camera_step[2])) {
                std::fprintf(stderr, "error: invalid value '%s' for '--camera-step': three finite numbers dx,dy,dz\n", v.c_str());
                return 2;
            }
        }
        else if (k == "--camera-move") { a.camera_move_given = true; a.camera_move = val(); }
        else if (k == "--instance-transform") {
            const std::string v = val();
            Args::InstanceTransform it{0, {0, 0, 0}, 0.0f, {1, 1, 1}};
            char tail = 0;
            int n = std::sscanf(v.c_str(), "%u:%f,%f,%f%c", &it.id, &it.t[0], &it.t[1], &it.t[2], &tail);
            bool ok = n == 4;
            if (n == 5 && tail == ':') {
                n = std::sscanf(v.c_str(), "%u:%f,%f,%f:%f%c", &it.id, &it.t[0], &it.t[1], &it.t[2], &it.ry_deg, &tail);
                ok = n == 5;
                if (n == 6 && tail == ':') ok = std::sscanf(v.c_str(), "%u:%f,%f,%f:%f:%f,%f,%f%c", &it.id, &it.t[0], &it.t[1], &it.t[2], &it.ry_deg, &it.s[0], &it.s[1], &it.s[2], &tail) == 8;
            }
            for (float f : {it.t[0], it.t[1], it.t[2], it.ry_deg, it.s[0], it.s[1], it.s[2]}) ok = ok && std::isfinite(f);
            ok = ok && !v.empty() && v[0] >= '0' && v[0] <= '9';
            for (const Args::InstanceTransform& o : a.instance_transforms) ok = ok && o.id != it.id;
            if (!ok) { std::fprintf(stderr, "error: invalid value '%s' for '--instance-transform': ID:tx,ty,tz[:ry_deg[:sx,sy,sz]], finite numbers, each ID once\n", v.c_str()); return 2; }
            a.instance_transforms.push_back(it);
        }
        else if (k == "--instance-step") {
            const std::string v = val();
            Args::InstanceTransform it{0, {0, 0, 0}, 0.0f, {1, 1, 1}};
            char tail = 0;
            int n = std::sscanf(v.c_str(), "%u:%f,%f,%f%c", &it.id, &it.t[0], &it.t[1], &it.t[2], &tail);
            bool ok = n == 4;
            if (n == 5 && tail == ':') ok = std::sscanf(v.c_str(), "%u:%f,%f,%f:%f%c", &it.id, &it.t[0], &it.t[1], &it.t[2], &it.ry_deg, &tail) == 5;
            for (float f : {it.t[0], it.t[1], it.t[2], it.ry_deg}) ok = ok && std::isfinite(f);
            ok = ok && !v.empty() && v[0] >= '0' && v[0] <= '9';
            for (const Args::InstanceTransform& o : a.instance_steps) ok = ok && o.id != it.id;
            if (!ok) { std::fprintf(stderr, "error: invalid value '%s' for '--instance-step': ID:tx,ty,tz[:ry_deg], finite numbers, each ID once\n", v.c_str()); return 2; }
            a.instance_steps.push_back(it);
        }
        else if (k == "--light-step") {
            const std::string v = val();
            Args::LightStep st{0, {0, 0, 0}, 1.0f};
            char tail = 0;
            int n = std::sscanf(v.c_str(), "%u:%f,%f,%f%c", &st.id, &st.d[0], &st.d[1], &st.d[2], &tail);
            bool ok = n == 4;
            if (n == 5 && tail == ':') ok = std::sscanf(v.c_str(), "%u:%f,%f,%f:%f%c", &st.id, &st.d[0], &st.d[1], &st.d[2], &st.gain, &tail) == 5;
            for (float f : {st.d[0], st.d[1], st.d[2], st.gain}) ok = ok && std::isfinite(f);
            ok = ok && !v.empty() && v[0] >= '0' && v[0] <= '9';
            for (const Args::LightStep& o : a.light_steps) ok = ok && o.id != st.id;
            if (!ok) { std::fprintf(stderr, "error: invalid value '%s' for '--light-step': ID:dx,dy,dz[:gain], finite numbers, each ID once\n", v.c_str()); return 2; }
            a.light_steps.push_back(st);
        }
        else if (k == "--emitter-gain") {
            const std::string v = val();
            Args::EmitterGain g{0, 1.0f};
            char tail = 0;
            bool ok = std::sscanf(v.c_str(), "%u:%f%c", &g.mat, &g.gain, &tail) == 2 && std::isfinite(g.gain) && !v.empty() && v[0] >= '0' && v[0] <= '9';
            for (const Args::EmitterGain& o : a.emitter_gains) ok = ok && o.mat != g.mat;
            if (!ok) { std::fprintf(stderr, "error: invalid value '%s' for '--emitter-gain': MAT:g, a finite number, each MAT once\n", v.c_str()); return 2; }
            a.emitter_gains.push_back(g);
        }
        else if (k == "--env-yaw-step") {
            const std::string v = val();
            char tail = 0;
            a.env_yaw_given = true;
            if (std::sscanf(v.c_str(), "%f%c", &a.env_yaw_step, &tail) != 1 || !std::isfinite(a.env_yaw_step)) { std::fprintf(stderr, "error: invalid value '%s' for '--env-yaw-step': a finite number of degrees\n", v.c_str()); return 2; }
        }
        else if (k == "--scene-edit") { a.scene_edit_given = true; a.scene_edit = val(); }
        else if (k == "--mesh-wave") {
            const std::string v = val();
            Args::MeshWave w{0, 0.0f, 0.0f, 0.0f};
            char tail = 0;
            int n = std::sscanf(v.c_str(), "%u:%f,%f%c", &w.geom, &w.amp, &w.wavelength, &tail);
            bool ok = n == 3;
            if (n == 4 && tail == ',') ok = std::sscanf(v.c_str(), "%u:%f,%f,%f%c", &w.geom, &w.amp, &w.wavelength, &w.phase_step, &tail) == 4;
            ok = ok && std::isfinite(w.amp) && std::isfinite(w.wavelength) && std::isfinite(w.phase_step) && w.wavelength != 0.0f;
            ok = ok && !v.empty() && v[0] >= '0' && v[0] <= '9';
            for (const Args::MeshWave& o : a.mesh_waves) ok = ok && o.geom != w.geom;
            if (!ok) { std::fprintf(stderr, "error: invalid value '%s' for '--mesh-wave': GEOM:amp,wavelength[,phase_step], finite numbers, a wavelength other than 0, each GEOM once\n", v.c_str()); return 2; }
            a.mesh_waves.push_back(w);
        }
        else if (k == "--instance-rebuild-above") {
            const std::string v = val();
            char tail = 0;
            a.instance_rebuild_given = true;
            if (std::sscanf(v.c_str(), "%f%c", &a.instance_rebuild_above, &tail) != 1 || !(a.instance_rebuild_above >= 0.0f) || !std::isfinite(a.instance_rebuild_above)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--instance-rebuild-above': 0 or a finite ratio above it\n", v.c_str());
                return 2;
            }
        }
        else if (k == "-h" || k == "--help") { usage(); return 0; }
        else { std::fprintf(stderr, "error: unexpected argument '%s'\n", k.c_str()); usage(); return 2; }
    }
    if (a.filter != "box") { std::fprintf(stderr, "error: invalid value '%s' for '--filter' (main.rs:33-37 offers only box)\n", a.filter.c_str()); return 2; }
    if (a.sampler != "random" && a.sampler != "sobol") { std::fprintf(stderr, "error: invalid value '%s' for '--sampler'\n", a.sampler.c_str()); return 2; }
    const bool gbuf = a.renderer == "position" || a.renderer == "depth";
    const bool aov = gbuf || a.renderer == "normal" || a.renderer == "albedo" || a.renderer == "shading-normal";   // (the primary-ray renderers)
    if (!aov && a.renderer != "pt" && a.renderer != "nee" && a.renderer != "mis") {
        std::fprintf(stderr, "error: invalid value '%s' for '--renderer' (main.rs:38-40: normal, albedo, pt, nee, mis; extensions: shading-normal, position, depth)\n", a.renderer.c_str());
        return 2;
    }
    // the display stage: refused here, before anything is loaded; mi355pt_display_device checks the struct again
    const bool display_on = !a.tone_map.empty() || a.auto_exposure;
    mi355pt_display_params_default(&display_stage.dp);
    if (!a.tone_map.empty()) {
        const char* names[5] = {"none", "reinhard", "reinhard-ext", "aces", "hable"};
        uint32_t t = 5;
        for (uint32_t i = 0; i < 5; ++i) if (a.tone_map == names[i]) t = i;
        if (t == 5) { std::fprintf(stderr, "error: invalid value '%s' for '--tone-map' (none, reinhard, reinhard-ext, aces, hable)\n", a.tone_map.c_str()); return 2; }
        display_stage.dp.tone = t;
    }
    if (display_on && (a.renderer != "pt" && a.renderer != "nee" && a.renderer != "mis")) {
        std::fprintf(stderr, "error: %s with --renderer %s: the display stage takes the film of a path renderer (pt, nee, mis)\n", a.auto_exposure ? "--auto-exposure" : "--tone-map", a.renderer.c_str());
        return 2;
    }
    if (display_on && a.gpus > 1) { std::fprintf(stderr, "error: %s with --gpus %d: the display stage runs on one GPU\n", a.auto_exposure ? "--auto-exposure" : "--tone-map", a.gpus); return 2; }
    if (a.white_given && display_stage.dp.tone != MI355PT_TONE_REINHARD_EXT && display_stage.dp.tone != MI355PT_TONE_HABLE) { std::fprintf(stderr, "error: --white needs --tone-map reinhard-ext or hable: the other curves have no white point\n"); return 2; }
    if (a.white_given && !(std::isfinite(a.white) && a.white >= 0x1p-16f && a.white <= 0x1p16f)) { std::fprintf(stderr, "error: --white must be in [2^-16, 2^16]\n"); return 2; }
    if ((a.exposure_key_given || a.exposure_adapt_given || a.exposure_trim_given) && !a.auto_exposure) {
        std::fprintf(stderr, "error: --exposure-key, --exposure-adapt and --exposure-trim need --auto-exposure: they are the meter's parameters\n");
        return 2;
    }
    if (a.exposure_key_given && !(std::isfinite(a.exposure_key) && a.exposure_key > 0.0f)) { std::fprintf(stderr, "error: --exposure-key must be finite and above 0\n"); return 2; }
    if (a.exposure_adapt_given && !(a.exposure_adapt >= 0.0f && a.exposure_adapt <= 1.0f)) { std::fprintf(stderr, "error: --exposure-adapt must be in [0, 1]\n"); return 2; }
    display_stage.on = display_on; display_stage.auto_exposure = a.auto_exposure;
    if (a.white_given) display_stage.dp.white = a.white;
    if (a.exposure_key_given) display_stage.dp.key = a.exposure_key;
    if (a.exposure_adapt_given) display_stage.dp.adapt = a.exposure_adapt;
    if (a.exposure_trim_given) { display_stage.dp.trim_low = a.exposure_trim[0]; display_stage.dp.trim_high = a.exposure_trim[1]; }
    // the bloom stage's flags: the sub-flags need --bloom, --bloom needs a path renderer on one GPU
    if (!a.bloom) {
        const char* sub = a.bloom_levels_given ? "--bloom-levels" : a.bloom_threshold_given ? "--bloom-threshold" : a.bloom_knee_given ? "--bloom-knee" : a.bloom_scatter_given ? "--bloom-scatter"
                          : a.bloom_intensity_given ? "--bloom-intensity" : a.bloom_additive ? "--bloom-additive" : a.bloom_no_firefly ? "--bloom-no-firefly" : nullptr;
        if (sub) { std::fprintf(stderr, "error: %s needs --bloom: it is a parameter of the bloom stage\n", sub); return 2; }
    } else {
        if (!a.bloom_additive && a.bloom_intensity_given && a.bloom_intensity > 1.0f) { std::fprintf(stderr, "error: --bloom-intensity above 1 needs --bloom-additive: the frame keeps 1 - intensity otherwise\n"); return 2; }
        if (aov) { std::fprintf(stderr, "error: --bloom with --renderer %s: the bloom stage takes the film of a path renderer (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
        if (a.gpus > 1) { std::fprintf(stderr, "error: --bloom with --gpus %d: the bloom stage runs on one GPU\n", a.gpus); return 2; }
        mi355pt_bloom_params& bp = display_stage.bp;
        mi355pt_bloom_params_default(&bp);
        if (a.bloom_levels_given) bp.levels = a.bloom_levels;
        if (a.bloom_no_firefly) bp.firefly = 0;
        if (a.bloom_knee_given) bp.knee = a.bloom_knee;
        if (a.bloom_scatter_given) bp.scatter = a.bloom_scatter;
        if (a.bloom_intensity_given) bp.intensity = a.bloom_intensity;
        bp.base = a.bloom_additive ? 1.0f : 1.0f - bp.intensity;
        bp.threshold = a.bloom_threshold_given ? a.bloom_threshold : (a.bloom_additive ? 1.0f : 0.0f);
        bp.exposure = display_stage.dp.exposure;
        display_stage.bloom_on = true;
    }
    // the robust film: refused here, before anything is loaded; mi355pt_robust_combine_device checks the struct again
    mi355pt_robust_params robust_params;
    mi355pt_robust_params_default(&robust_params);
    if ((!a.robust_mode.empty() || a.robust_scale_given) && !a.robust_given) { std::fprintf(stderr, "error: --robust-mode and --robust-scale need --robust-buckets: they are the combination's parameters\n"); return 2; }
    if (a.robust_given) {
        const uint32_t K = a.robust_buckets;
        if (K != 4 && K != 8 && K != 16 && K != 32) { std::fprintf(stderr, "error: invalid value '%u' for '--robust-buckets' (4, 8, 16 or 32)\n", K); return 2; }
        if (aov) { std::fprintf(stderr, "error: --robust-buckets with --renderer %s: the robust film is for the path renderers (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
        if (a.gpus > 1) { std::fprintf(stderr, "error: --robust-buckets with --gpus %d: the robust film runs on one GPU\n", a.gpus); return 2; }
        if (a.adaptive_threshold != 0.0f) { std::fprintf(stderr, "error: --robust-buckets with --adaptive-threshold: the buckets take one sample count per frame\n"); return 2; }
        if (a.half_res) { std::fprintf(stderr, "error: --robust-buckets with --half-res: the buckets are rendered at full size\n"); return 2; }
        if (a.temporal) { std::fprintf(stderr, "error: --robust-buckets with --temporal-frames: the robust film is one frame\n"); return 2; }
        if (a.spp == 0 || a.spp % K != 0) { std::fprintf(stderr, "error: --robust-buckets %u needs --spp to be a multiple of it above 0 (got --spp %u)\n", K, a.spp); return 2; }
        if (!a.robust_mode.empty()) {
            const char* names[3] = {"mean", "mom", "gmon"};      // MI355PT_ROBUST_*
            uint32_t m = 3;
            for (uint32_t i = 0; i < 3; ++i) if (a.robust_mode == names[i]) m = i;
            if (m == 3) { std::fprintf(stderr, "error: invalid value '%s' for '--robust-mode' (gmon, mom, mean)\n", a.robust_mode.c_str()); return 2; }
            robust_params.mode = m;
        }
        if (a.robust_scale_given && !(std::isfinite(a.robust_scale) && a.robust_scale >= 0.0f)) { std::fprintf(stderr, "error: --robust-scale must be finite and not below 0\n"); return 2; }
        if (a.robust_scale_given) robust_params.gini_scale = a.robust_scale;
    }
    if (a.flow && !a.temporal) { std::fprintf(stderr, "error: --flow needs --temporal-frames: it carries the accumulation across the frames' moves\n"); return 2; }
    if ((a.temporal_budget || a.temporal_budget_max_given) && !a.temporal) { std::fprintf(stderr, "error: --temporal-budget and --temporal-budget-max-spp need --temporal-frames: they budget its frames' samples\n"); return 2; }
    if (a.temporal_budget_max_given && !a.temporal_budget) { std::fprintf(stderr, "error: --temporal-budget-max-spp needs --temporal-budget\n"); return 2; }
    if (a.temporal_budget && a.half_res) { std::fprintf(stderr, "error: --temporal-budget with --half-res: the budget's tiles would be the low frame's\n"); return 2; }
    if (a.temporal_budget) {
        const auto pow2 = [](uint32_t v) { return v != 0 && (v & (v - 1)) == 0; };
        if (!(std::isfinite(a.temporal_budget_target) && a.temporal_budget_target >= 1.0f)) { std::fprintf(stderr, "error: --temporal-budget must be finite and at least 1 (the history length a tile should reach)\n"); return 2; }
        if (a.spp < 2 || !pow2(a.spp) || a.spp > (1u << 28)) { std::fprintf(stderr, "error: --temporal-budget needs a --spp that is a power of two, at least 2: it is the budget's base count\n"); return 2; }
        if (a.temporal_budget_max_given && (!pow2(a.temporal_budget_max_spp) || a.temporal_budget_max_spp < a.spp)) { std::fprintf(stderr, "error: --temporal-budget-max-spp must be a power of two, at least --spp\n"); return 2; }
    }
    if (a.flow && a.half_res) { std::fprintf(stderr, "error: --flow with --half-res: the flow-aware accumulation runs at full size only\n"); return 2; }
    if (a.half_res_albedo && !a.half_res) { std::fprintf(stderr, "error: --half-res-albedo needs --half-res: it demodulates the film that --half-res upsamples\n"); return 2; }
    if (a.half_res && aov) { std::fprintf(stderr, "error: --half-res with --renderer %s: half-resolution rendering is for the path renderers (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
    if (a.half_res && (a.width == 0 || a.height == 0 || (a.width & 1u) != 0 || (a.height & 1u) != 0)) { std::fprintf(stderr, "error: --half-res needs an even --width and --height above 0 (got %u x %u)\n", a.width, a.height); return 2; }
    if (a.half_res && a.gpus > 1) { std::fprintf(stderr, "error: --half-res with --gpus %d: half-resolution rendering runs on one GPU\n", a.gpus); return 2; }
    if (a.half_res && a.denoise) { std::fprintf(stderr, "error: --half-res with --denoise: the upsampled pair goes to --denoise-variance\n"); return 2; }
    if (a.half_res && a.adaptive_threshold != 0.0f) { std::fprintf(stderr, "error: --half-res with --adaptive-threshold: half-resolution rendering takes one sample count per frame\n"); return 2; }
    if (a.half_res && (a.spp == 0 || a.denoise_guide_spp == 0)) { std::fprintf(stderr, "error: --half-res needs --spp and --denoise-guide-spp above 0\n"); return 2; }
    if (a.instance_rebuild_given && a.instance_transforms.empty() && a.mesh_waves.empty()) { std::fprintf(stderr, "error: --instance-rebuild-above needs --instance-transform or --mesh-wave: it is the move's threshold\n"); return 2; }
    if (!a.mesh_waves.empty()) {
        if (a.temporal && !a.flow) { std::fprintf(stderr, "error: --mesh-wave with --temporal-frames: the temporal reprojection assumes rigid motion per instance (no motion vectors for deforming meshes yet)\n"); return 2; }
        if (a.gpus > 1) { std::fprintf(stderr, "error: --mesh-wave with --gpus %d: a scene built over several GPUs is not deformed\n", a.gpus); return 2; }
        if (a.renderer == "shading-normal") { std::fprintf(stderr, "error: --mesh-wave with --renderer shading-normal: pt, nee, mis, normal, albedo, position or depth\n"); return 2; }
        std::sort(a.mesh_waves.begin(), a.mesh_waves.end(), [](const Args::MeshWave& x, const Args::MeshWave& y) { return x.geom < y.geom; });
    }
    if (!a.instance_steps.empty()) {
        for (const Args::InstanceTransform& st : a.instance_steps)
            for (const Args::InstanceTransform& it : a.instance_transforms)
                if (st.id == it.id) { std::fprintf(stderr, "error: --instance-step and --instance-transform both name instance %u: one of them\n", st.id); return 2; }
        if (!a.temporal) { std::fprintf(stderr, "error: --instance-step needs --temporal-frames: it moves the instance between the frames\n"); return 2; }
        if (a.half_res) { std::fprintf(stderr, "error: --instance-step with --half-res: the motion-aware accumulation runs at full size only\n"); return 2; }
        std::sort(a.instance_steps.begin(), a.instance_steps.end(), [](const Args::InstanceTransform& x, const Args::InstanceTransform& y) { return x.id < y.id; });
    }
    if (!a.instance_transforms.empty()) {
        if (a.temporal) { std::fprintf(stderr, "error: --instance-transform with --temporal-frames: the temporal reprojection assumes a static world (no object motion vectors)\n"); return 2; }
        if (a.gpus > 1) { std::fprintf(stderr, "error: --instance-transform with --gpus %d: a scene built over several GPUs is not moved\n", a.gpus); return 2; }
        if (a.renderer == "shading-normal") { std::fprintf(stderr, "error: --instance-transform with --renderer shading-normal: pt, nee, mis, normal, albedo, position or depth\n"); return 2; }
        std::sort(a.instance_transforms.begin(), a.instance_transforms.end(), [](const Args::InstanceTransform& x, const Args::InstanceTransform& y) { return x.id < y.id; });
    }
    if (a.camera_step_given && !a.temporal) { std::fprintf(stderr, "error: --camera-step needs --temporal-frames: it moves the camera between the frames\n"); return 2; }
    if (a.camera_move != "rebuild" && a.camera_move != "rebase") { std::fprintf(stderr, "error: invalid value '%s' for '--camera-move' (rebuild or rebase)\n", a.camera_move.c_str()); return 2; }
    if (a.camera_move_given && !a.temporal) { std::fprintf(stderr, "error: --camera-move needs --temporal-frames: it says how the scene follows the camera between the frames\n"); return 2; }
    if (a.scene_edit != "inplace" && a.scene_edit != "rebuild") { std::fprintf(stderr, "error: invalid value '%s' for '--scene-edit' (inplace or rebuild)\n", a.scene_edit.c_str()); return 2; }
    if ((a.editing() || a.scene_edit_given) && !a.temporal) { std::fprintf(stderr, "error: --light-step, --emitter-gain, --env-yaw-step and --scene-edit need --temporal-frames: they change the scene between the frames\n"); return 2; }
    if (a.scene_edit_given && !a.editing()) { std::fprintf(stderr, "error: --scene-edit says how --light-step, --emitter-gain and --env-yaw-step reach the scene: give one of them\n"); return 2; }
    if (a.editing() && !a.temporal_rectify) std::fprintf(stderr, "note: without --temporal-rectify the plain accumulation averages the change of light over its history\n");
    std::sort(a.light_steps.begin(), a.light_steps.end(), [](const Args::LightStep& x, const Args::LightStep& y) { return x.id < y.id; });
    std::sort(a.emitter_gains.begin(), a.emitter_gains.end(), [](const Args::EmitterGain& x, const Args::EmitterGain& y) { return x.mat < y.mat; });
    if (a.temporal && a.temporal_frames == 0) { std::fprintf(stderr, "error: --temporal-frames must be above 0\n"); return 2; }
    if (a.temporal && aov) { std::fprintf(stderr, "error: --temporal-frames with --renderer %s: temporal accumulation is for the path renderers (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
    if (a.temporal && a.gpus > 1) { std::fprintf(stderr, "error: --temporal-frames with --gpus %d: temporal accumulation runs on one GPU\n", a.gpus); return 2; }
    if (a.temporal && a.denoise) { std::fprintf(stderr, "error: --temporal-frames with --denoise: the accumulated pair goes to --denoise-variance\n"); return 2; }
    if (a.temporal && a.adaptive_threshold != 0.0f) { std::fprintf(stderr, "error: --temporal-frames with --adaptive-threshold: temporal accumulation takes one sample count per frame\n"); return 2; }
    if (a.temporal && (a.spp == 0 || a.denoise_guide_spp == 0)) { std::fprintf(stderr, "error: --temporal-frames needs --spp and --denoise-guide-spp above 0\n"); return 2; }
    if ((a.temporal_rectify || a.temporal_rectify_radius_given || a.temporal_rectify_gamma_given) && !a.temporal) {
        std::fprintf(stderr, "error: --temporal-rectify, --temporal-rectify-radius and --temporal-rectify-gamma need --temporal-frames: they rectify its history\n");
        return 2;
    }
    if ((a.temporal_rectify_radius_given || a.temporal_rectify_gamma_given) && !a.temporal_rectify) {
        std::fprintf(stderr, "error: --temporal-rectify-radius and --temporal-rectify-gamma need --temporal-rectify\n");
        return 2;
    }
    if (a.temporal_rectify_radius_given && (a.temporal_rectify_radius < 1 || a.temporal_rectify_radius > 3)) {
        std::fprintf(stderr, "error: --temporal-rectify-radius must be 1, 2 or 3\n");
        return 2;
    }
    if (a.temporal_rectify_gamma_given && !(std::isfinite(a.temporal_rectify_gamma) && a.temporal_rectify_gamma > 0.0f)) {
        std::fprintf(stderr, "error: --temporal-rectify-gamma must be finite and above 0\n");
        return 2;
    }
    if (gbuf && (a.output.size() < 4 || a.output.compare(a.output.size() - 4, 4, ".pfm") != 0)) {
        std::fprintf(stderr, "error: --renderer %s writes float values: -o must end in .pfm (got '%s')\n", a.renderer.c_str(), a.output.c_str());
        return 2;
    }
    if (a.fused_guides && !a.denoise && !a.denoise_variance) { std::fprintf(stderr, "error: --fused-guides needs --denoise or --denoise-variance: it renders their guide films\n"); return 2; }
    if (aov && a.gpus > 1) { std::fprintf(stderr, "error: --gpus %d with --renderer %s: the AOV renderers run on one GPU\n", a.gpus, a.renderer.c_str()); return 2; }
    if (a.denoise && aov) { std::fprintf(stderr, "error: --denoise with --renderer %s: the denoiser filters the frame of a path renderer (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
    if (a.denoise && a.gpus > 1) { std::fprintf(stderr, "error: --denoise with --gpus %d: the denoiser runs on one GPU\n", a.gpus); return 2; }
    if (a.denoise && (a.denoise_guide_spp == 0 || a.spp == 0)) { std::fprintf(stderr, "error: --denoise needs --spp and --denoise-guide-spp above 0\n"); return 2; }
    if (a.denoise_variance && a.denoise) { std::fprintf(stderr, "error: --denoise-variance with --denoise: one filter or the other\n"); return 2; }
    if (a.denoise_variance && aov) { std::fprintf(stderr, "error: --denoise-variance with --renderer %s: the denoiser filters the frame of a path renderer (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
    if (a.denoise_variance && a.gpus > 1) { std::fprintf(stderr, "error: --denoise-variance with --gpus %d: the denoiser runs on one GPU\n", a.gpus); return 2; }
    if (a.denoise_variance && (a.denoise_guide_spp == 0 || a.spp == 0 || (a.spp & 1u) != 0)) { std::fprintf(stderr, "error: --denoise-variance needs an even --spp (the half film holds the first half of the samples) and --denoise-guide-spp above 0\n"); return 2; }
    if (a.denoise_sigma_lum != 0.0f && (!a.denoise_variance || !(a.denoise_sigma_lum > 0.0f) || !std::isfinite(a.denoise_sigma_lum))) { std::fprintf(stderr, "error: --denoise-sigma-lum needs --denoise-variance and a finite value above 0\n"); return 2; }
    const bool adaptive = a.adaptive_threshold != 0.0f;
    if (!adaptive && !a.spp_map.empty()) { std::fprintf(stderr, "error: --spp-map needs --adaptive-threshold\n"); return 2; }
    if (adaptive && aov) { std::fprintf(stderr, "error: --adaptive-threshold with --renderer %s: adaptive sampling is for the path renderers (pt, nee, mis)\n", a.renderer.c_str()); return 2; }
    if (adaptive && a.gpus > 1) { std::fprintf(stderr, "error: --adaptive-threshold with --gpus %d: adaptive sampling runs on one GPU\n", a.gpus); return 2; }
    if (adaptive && (!(a.adaptive_threshold > 0.0f) || !(a.adaptive_dark_eps > 0.0f) || a.adaptive_min_spp < 2 || (a.adaptive_min_spp & (a.adaptive_min_spp - 1)) != 0 ||
                     (a.spp & (a.spp - 1)) != 0 || a.spp < a.adaptive_min_spp)) {
        std::fprintf(stderr, "error: --adaptive-threshold and --adaptive-dark-eps must be above 0, --adaptive-min-spp a power of two from 2, --spp (the maximum) a power of two from --adaptive-min-spp\n");
        return 2;
    }
    try {
        Camera camera(45.0f, a.width, a.height);                                        // main.rs:59-68
        Scene scene;
        switch (a.scene) {                                                              // main.rs:70-92
            case 0: load_scene_0(scene, camera); break;
            case 1: load_scene_1(scene, camera); break;
            case 2: load_scene_2(scene, camera); break;
            case 3: load_scene_3(scene, camera); break;
            case 4: load_scene_4(scene, camera); break;
            case 5: load_scene_5(scene, camera); break;
            case 9: load_scene_9(scene, camera); break;
            case 12: load_scene_12(scene, camera); break;
            case 13: load_scene_13(scene, camera); break;
            case 14: load_scene_14(scene, camera); break;
            case 15: load_scene_15(scene, camera); break;
            case 16: load_scene_16_18(scene, camera, false); break;
            case 18: load_scene_16_18(scene, camera, true); break;
            case 6: load_scene_6(scene, camera); break;
            case 7: load_scene_7(scene, camera); break;
            case 11: load_scene_11(scene, camera); break;
            case 8: load_scene_8(scene, camera); break;
            case 10: load_scene_10(scene, camera); break;
            case 17: load_scene_17(scene, camera); break;
            case 19: load_scene_19(scene, camera); break;
            default: std::fprintf(stderr, "scene %u is outside the MI355X hot-path scope (scenes 0-19)\n", a.scene); return 2;
        }
        for (const Args::InstanceTransform& it : a.instance_transforms) {
            if (it.id >= scene.instance_count()) { std::fprintf(stderr, "error: invalid value for '--instance-transform': scene %u has no instance %u (%u instances)\n", a.scene, it.id, scene.instance_count()); return 2; }
            scene.set_instance_dynamic(it.id);
        }
        for (const Args::InstanceTransform& it : a.instance_steps) {
            if (it.id >= scene.instance_count()) { std::fprintf(stderr, "error: invalid value for '--instance-step': scene %u has no instance %u (%u instances)\n", a.scene, it.id, scene.instance_count()); return 2; }
            scene.set_instance_dynamic(it.id);
        }
        for (const Args::LightStep& st : a.light_steps)
            if (st.id >= scene.light_count()) { std::fprintf(stderr, "error: invalid value for '--light-step': scene %u has no delta light %u (%u delta lights)\n", a.scene, st.id, scene.light_count()); return 2; }
        for (const Args::EmitterGain& g : a.emitter_gains)
            if (!scene.has_material(g.mat) || scene.material_desc(g.mat).type != MI355PT_MAT_EMISSIVE) { std::fprintf(stderr, "error: invalid value for '--emitter-gain': material %u of scene %u is not an emissive material\n", g.mat, a.scene); return 2; }
        if (a.env_yaw_given && scene.env_count() == 0) { std::fprintf(stderr, "error: --env-yaw-step: scene %u has no environment light\n", a.scene); return 2; }
        for (const Args::MeshWave& w : a.mesh_waves)
            if (w.geom >= scene.mesh_count()) { std::fprintf(stderr, "error: invalid value for '--mesh-wave': scene %u has no mesh %u (%u meshes)\n", a.scene, w.geom, scene.mesh_count()); return 2; }
        std::puts("Start build scene.");                                                // main.rs:103-109
        auto t0 = std::chrono::steady_clock::now();
        if (a.gpus > 1) scene.build_multi(camera, a.gpus); else scene.build(camera);
        if (!a.instance_transforms.empty()) {
            std::vector<uint32_t> ids; std::vector<float> matrices(16 * a.instance_transforms.size());
            for (size_t k = 0; k < a.instance_transforms.size(); ++k) {
                ids.push_back(a.instance_transforms[k].id);
                instance_transform_matrix(a.instance_transforms[k], scene.instance_transform(ids.back()), &matrices[16 * k]);
            }
            const mi355pt_instance_move_result mr = scene.move_instances(camera, ids, matrices, a.instance_rebuild_above);
            std::fprintf(stderr, "instance move: rebuilt=%u reason=%u launches=%u sah=%.6g\xe2\x86\x92%.6g host_ms=%.3f device_ms=%.3f\n", mr.rebuilt, mr.reason, mr.launches,
                         (double)mr.sah_built, (double)mr.sah_after, mr.host_ms, mr.device_ms);
        }
        if (!a.mesh_waves.empty() && !a.flow) {      // (--flow: the frames deform, render_temporal)
            std::vector<uint32_t> geoms; std::vector<std::vector<float>> pos, nrm;
            for (const Args::MeshWave& w : a.mesh_waves) {
                geoms.push_back(w.geom);
                pos.push_back(waved_positions(w, scene.mesh(w.geom).pos));
                nrm.push_back(area_weighted_normals(scene.mesh(w.geom), pos.back()));
            }
            const mi355pt_instance_move_result mr = scene.deform_meshes(camera, geoms, pos, nrm, a.instance_rebuild_above);
            std::fprintf(stderr, "mesh deform: rebuilt=%u reason=%u launches=%u sah=%.6g\xe2\x86\x92%.6g host_ms=%.3f device_ms=%.3f\n", mr.rebuilt, mr.reason, mr.launches,
                         (double)mr.sah_built, (double)mr.sah_after, mr.host_ms, mr.device_ms);
        }
        std::printf("Finish build scene: %.3f seconds.\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());

        RendererArgs args{a.width, a.height, a.spp, a.seed, &scene, &camera};
        SrgbRenderer r;
        if (a.renderer == "pt") r = SrgbRendererPt(args, 1.0f, a.max_depth);            // main.rs:188-233: exposure 1.0, Reinhard
        else if (a.renderer == "nee") r = SrgbRendererNee(args, 1.0f, a.max_depth);
        else if (a.renderer == "mis") r = SrgbRendererMis(args, 1.0f, a.max_depth);
        else if (a.renderer == "normal") r = NormalRenderer(args);                      // main.rs:155-170
        else if (a.renderer == "albedo") r = AlbedoRenderer(args);                      // main.rs:171-186
        else r = ShadingNormalRenderer(args);                                           // (position / depth: its params; the G-buffer pass renders)
        RendererImage image(a.width, a.height, r);
        std::puts("Start rendering...");                                                // main.rs:166-172
        t0 = std::chrono::steady_clock::now();
        const SamplerKind sampler = a.sampler == "sobol" ? SamplerKind::ZSobol : SamplerKind::Random;
        double kernel_s = 0.0;
        if (gbuf) kernel_s = render_gbuffer_float(scene, camera, image.params(sampler, a.albedo_lut), a.renderer == "depth", image.pixels_mut());
        else if (a.half_res) kernel_s = render_half_res(scene, camera, image.params(sampler, a.albedo_lut), a, image.pixels_mut());
        else if (a.temporal) kernel_s = render_temporal(scene, camera, image.params(sampler, a.albedo_lut), a, image.pixels_mut());
        else if (adaptive) render_adaptive(scene, camera, image.params(sampler, a.albedo_lut), a, image.pixels_mut());
        else if (a.robust_given) kernel_s = render_robust(scene, camera, image.params(sampler, a.albedo_lut), a, robust_params, image.pixels_mut());
        else if (a.denoise_variance) kernel_s = render_denoised_variance(scene, camera, image.params(sampler, a.albedo_lut), a.denoise_guide_spp, a.fused_guides, a.denoise_sigma_lum, image.pixels_mut());
        else kernel_s = a.denoise ? render_denoised(scene, camera, image.params(sampler, a.albedo_lut), a.denoise_guide_spp, a.fused_guides, image.pixels_mut())
                                    : (display_stage.on || display_stage.bloom_on ? render_displayed(scene, camera, image.params(sampler, a.albedo_lut), image.pixels_mut()) : image.render(sampler, a.albedo_lut));
        double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("Finish rendering: %.3f seconds.\n", wall);
        if (kernel_s > 0.0 && a.half_res) std::printf("(beauty launches at %u x %u: device %.3f s; the two G-buffers, the upsample and what follows it are in the wall time above)\n", a.width / 2, a.height / 2, kernel_s);
        else if (kernel_s > 0.0 && a.temporal) std::printf("(beauty launches of %u frames: device %.3f s; the G-buffer, the accumulation and the scene builds are in the wall time above)\n", a.temporal_frames, kernel_s);
        else if (kernel_s > 0.0 && a.robust_given) std::printf("(bucket launches: device %.3f s, %.1f Msamples/s; the combination and what follows it are in the wall time above)\n", kernel_s, (double)a.width * a.height * a.spp / kernel_s / 1e6);
        else if (kernel_s > 0.0 && (a.denoise || a.denoise_variance)) std::printf("(beauty launch alone: device %.3f s, %.1f Msamples/s; the guide films and the filter are in the wall time above)\n", kernel_s, (double)a.width * a.height * a.spp / kernel_s / 1e6);
        else if (kernel_s > 0.0) std::printf("(device %.3f s, %.1f Msamples/s)\n", kernel_s, (double)a.width * a.height * a.spp / kernel_s / 1e6);
        display_stage.release();
        if (gbuf) write_pfm(a.output, image.pixels().data(), a.width, a.height); else image.save(a.output);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mi355pt: %s\n", e.what());
        return 1;
    }
    return 0;
}
