/*
 * mi355pt_denoise.h — the denoiser block of the C ABI (included by mi355pt.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference writes its noisy frame and its two AOV images and stops.  This is the post-process
 * that combines them on the device: an edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous
 * Wavelet Transform for fast Global Illumination Filtering", HPG 2010) over the LINEAR film of a path renderer, guided by the albedo and
 * shading-normal films.
 *
 * Inputs are row-major W x H x 3 f32 buffers of linear SUMS, exactly what mi355pt_render_accum_device and mi355pt_render_aov_accum_device
 * write: beauty B over spp_beauty samples (required), albedo A (MI355PT_AOV_ALBEDO) over spp_albedo and shading normal N
 * (MI355PT_AOV_SHADING_NORMAL) over spp_normal (either may be NULL: its term is then absent).
 *
 * Prepass, per pixel and channel:  c = B / spp_beauty, a non-finite c becomes 0, then c = max(c, 0);  a = max(A / spp_albedo, 0);
 *   n = 2 N / spp_normal - 1 (not renormalised);  the pixel is BACKGROUND when N is given and its three sums are exactly 0 (every sample
 *   missed);  irr = c / (a + albedo_eps) when A is given, else c.
 * Level i = 0 .. levels-1, step s = 2^i, for each non-background pixel p: the taps are q = p + s (dx, dy), dx, dy in -2 .. 2; a tap
 *   outside the image is skipped, a background tap has weight 0;
 *     d = |t(irr_p) - t(irr_q)|^2 4^i / sigma_color^2 + |n_p - n_q|^2 / sigma_normal^2 + |a_p - a_q|^2 / sigma_albedo^2,  t(x) = x / (1 + x)
 *     w = h[dx] h[dy] exp(-d),  h = (1/16, 1/4, 3/8, 1/4, 1/16),        irr'_p = sum w irr_q / sum w
 *   (the centre tap makes sum w > 0).  Background pixels keep their value.  The guides are the same on every level.
 * Output, W x H x 3 f32: irr_final (a + albedo_eps) (irr_final without A) on non-background pixels, c bit for bit on background pixels:
 *   a linear MEAN, i.e. a film with spp = 1 for mi355pt_film_resolve_device — tone mapping stays where it is.
 *
 * The beauty film may hold anything (NaN, +-inf and negative values are cleaned as above).  The guide films must be FINITE, and c / (a +
 * albedo_eps) must not overflow binary32: otherwise the affected pixels and their neighbours are unspecified (they may come back NaN).
 *
 * Guides want more samples than the frame: at 4 spp the albedo film carries its own spectral noise and the albedo term then hurts, which
 * is why every buffer has its own spp.
 */
#ifndef MI355PT_DENOISE_H
#define MI355PT_DENOISE_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_denoise_params {
    uint32_t levels; /* 1 .. 8 */
    float sigma_color, sigma_normal, sigma_albedo, albedo_eps; /* all finite and > 0 */
} mi355pt_denoise_params;

/* levels 5, sigma_color 1.0, sigma_normal 0.5, sigma_albedo 0.3, albedo_eps 0.01 */
void mi355pt_denoise_params_default(mi355pt_denoise_params* out);
/* Bytes of device scratch mi355pt_denoise_device needs for a width x height frame: four 16-byte records per pixel (two irr buffers that
 * ping-pong, the normal + background flag, the albedo).  0 when the product does not fit a size_t. */
size_t mi355pt_denoise_scratch_bytes(uint32_t width, uint32_t height);
/* The filter on device buffers.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing, synchronises
 * nothing, uses no atomics: two runs are bit-equal.  d_scratch (16-byte aligned, scratch_bytes >= mi355pt_denoise_scratch_bytes) is
 * overwritten.  Returns MI355PT_E_INVALID — before anything touches the device — when: levels is outside 1 .. 8; a sigma or albedo_eps is
 * not finite or not > 0 (a zero-initialised params struct is refused, never interpreted); the spp of a given buffer is 0; width or height
 * is 0 (or the frame has more than 2^31 - 1 blocks of 64 x 4 pixels); d_beauty, d_out, the params pointer or d_scratch is NULL; the scratch
 * is too small or not 16-byte aligned; d_out equals an input pointer. */
int mi355pt_denoise_device(const float* d_beauty, uint32_t spp_beauty, const float* d_albedo, uint32_t spp_albedo, const float* d_normal,
                           uint32_t spp_normal, uint32_t width, uint32_t height, const mi355pt_denoise_params* params, void* d_scratch,
                           size_t scratch_bytes, float* d_out, void* hip_stream);
/* The same with host buffers: allocates the device buffers and the scratch, copies, runs mi355pt_denoise_device on the default stream,
 * synchronises and copies the result to `out`.  Same argument checks (scratch aside), before any allocation. */
int mi355pt_denoise(const float* beauty, uint32_t spp_beauty, const float* albedo, uint32_t spp_albedo, const float* normal,
                    uint32_t spp_normal, uint32_t width, uint32_t height, const mi355pt_denoise_params* params, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_DENOISE_H */
