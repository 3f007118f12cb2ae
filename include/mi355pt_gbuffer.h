/*
 * mi355pt_gbuffer.h — the G-buffer block of the C ABI (included by mi355pt.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart as a renderer: ONE primary-ray pass that writes up to four films from the SAME rays, where
 * mi355pt_render_aov_accum_device walks the scene once per film.  The albedo film is AlbedoRenderer::render
 * (renderer/albedo_renderer.rs:30-69) sample for sample — bit for bit the film of MI355PT_AOV_ALBEDO.
 *
 * The text below is normative: tests/gbuffer_reference.cpp restates it on the CPU oracle.
 *
 * Per pixel and sample index the schedule is the albedo renderer's, WHICHEVER films are requested — so a film never depends on which
 * other films were asked for:
 *     get_1d() -> SampledWavelengths::new_uniform;  get_2d_pixel();  camera.sample_ray, not moved forward (no epsilon);  the closest hit;
 *     one surface interaction in render space (the camera is the origin).
 * A film is requested when its pointer in mi355pt_gbuffer_films is non-NULL; a film that is not requested is never read or written.
 * Each film is a row-major W x H x 3 f32 buffer of linear SUMS (y down), and a sample adds:
 *     albedo          exactly what MI355PT_AOV_ALBEDO adds: sample_albedo_spectrum(uv, lambda) of a BSDF material times
 *                     presets::cie_illum_d6500() through Sensor::add_sample with exposure 1.  Emitters and misses add nothing.
 *     shading_normal  ns * 0.5 + 0.5 of the render-space shading normal for EVERY hit, emitters included (the expression of
 *                     MI355PT_AOV_SHADING_NORMAL).  A miss adds 0.
 *     position        the render-space hit position.  A miss adds 0.
 *     hit             (t_hit, 1, emitter ? 1 : 0), t_hit the distance along the unit ray.  A miss adds 0.  So .y is the pixel's hit count,
 *                     .x / .y the mean distance, .z / .y the emitter share, and spp - .y the misses.
 * A pixel's sums START from the values in the films and take the samples in index order, one binary32 add each: [0, a) then [a, b) leaves
 * the bits of [0, b), the shards of a frame compose to the frame, and two runs are bit-equal (no atomics).
 *
 * Because a miss adds 0, sum / spp is biased towards 0 on partly covered pixels (silhouettes against the environment).
 * mi355pt_gbuffer_normalize_device divides that out: film / hit.y.
 */
#ifndef MI355PT_GBUFFER_H
#define MI355PT_GBUFFER_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the films of one call: device pointers for the _device entry point, host pointers for mi355pt_render_gbuffer; NULL = not wanted */
typedef struct mi355pt_gbuffer_films {
    float *albedo, *shading_normal, *position, *hit;
} mi355pt_gbuffer_films;

/* Adds the sums of sample indices [sample_begin, sample_end) to the requested films (device, W*H*3 f32 each) for the 8x8 tiles of the shard
 * in `p`, other pixels untouched: one launch.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream).
 * Of mi355pt_params, spp, seed, sampler, shard_index and shard_count are honoured; strategy, max_depth, exposure and albedo_lut are
 * ignored; rr_gate_slack must be 0 as everywhere; collect_stats != 0 returns MI355PT_E_INVALID (there is no instrumented kernel) — the
 * rules of mi355pt_render_aov.  `illuminant_lut` is the LUT470 id of presets::cie_illum_d6500() in this scene: needed when `albedo` is
 * requested, ignored otherwise.
 * Returns MI355PT_E_INVALID — before anything touches the device, and before the scene is looked at — when: `films` is NULL; all four film
 * pointers are NULL; two film pointers are equal; sample_end > spp or sample_begin > sample_end; the frame is zero-sized; a scene, camera
 * or params pointer is NULL; illuminant_lut is not a LUT470 id of the scene and `albedo` is requested.  sample_begin == sample_end is a
 * valid empty range: nothing is launched.  Then the checks of mi355pt_render_aov (MI355PT_E_NOT_BUILT for a scene that is not built, the
 * camera-position and device contract).
 * `stats`, when given, receives samples, closest_rays, closest_hits, kernel_ms and launches; the rest is 0. */
int mi355pt_render_gbuffer_accum_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut,
                                        uint32_t sample_begin, uint32_t sample_end, const mi355pt_gbuffer_films* films, void* hip_stream,
                                        mi355pt_stats* stats /* NULL ok; non-NULL synchronises the stream */);
/* Coverage-normalised means on device buffers: d_out[i] = d_film[i] / hit.y of the value's pixel where hit.y > 0, else 0 (n_pixels * 3
 * values; d_hit is the `hit` film of the same frame).  position and shading_normal films give the mean over the samples that hit; the hit
 * film itself gives depth = hit.x / hit.y in .x.  One binary32 division per value.  Asynchronous on `hip_stream`.  MI355PT_E_INVALID when a
 * pointer is NULL or d_out equals d_film or d_hit. */
int mi355pt_gbuffer_normalize_device(const float* d_film, const float* d_hit, uint32_t n_pixels, float* d_out, void* hip_stream);
/* The whole pass with host buffers: allocates and zeroes a device film per requested film of `out` (host, W*H*3 f32 each, NULL = not
 * wanted), runs mi355pt_render_gbuffer_accum_device over [0, spp) on the default stream and returns MEANS: sum / spp for shading_normal,
 * position and hit; for albedo what mi355pt_aov_resolve_device(MI355PT_AOV_ALBEDO) gives (mean, clip at 0 from below, sRGB OETF).  Same
 * argument checks, before any allocation. */
int mi355pt_render_gbuffer(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t illuminant_lut,
                           const mi355pt_gbuffer_films* out, mi355pt_stats* stats /* NULL ok */);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_GBUFFER_H */
