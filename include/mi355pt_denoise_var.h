/*
 * mi355pt_denoise_var.h — the variance-guided denoiser block of the C ABI (included by mi355pt.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart, and a SECOND filter beside the one of mi355pt_denoise.h, which stays as it is.  That one stops at
 * colour edges with a fixed sigma_color and so keeps blurring as the frame converges; this one measures the noise.  The film F of n samples
 * and the half film H of its first n / 2 (the pair the adaptive driver of mi355pt_adaptive.h keeps: "F = the sum of [0, n), H = the sum of
 * [0, n / 2)") give two independent half means per pixel, and so the variance of the pixel's mean at no extra cost.  An a-trous filter in
 * the manner of SVGF (Schied et al.: "Spatiotemporal Variance-Guided Filtering", HPG 2017) divides the luminance distance of a tap by the
 * local standard deviation and carries the variance through the levels: it fades out as the frame converges.
 *
 * The text below is normative: tests/denoise_var_reference.py restates it in NumPy.  All arithmetic is binary32, every operation rounded
 * on its own.
 *
 * Inputs are row-major W x H x 3 f32 buffers of linear SUMS: beauty B and half film H (both required), albedo A over spp_albedo and
 * shading normal N over spp_normal (either may be NULL: its term is then absent), as in mi355pt_denoise.h.
 * Sample count n of a pixel: spp_beauty when d_tile_spp is NULL; otherwise the u32 of the pixel's 8x8 tile, tile t = (t % tiles_x,
 *   t / tiles_x), tiles_x = ceil(W / 8) (the tiles of mi355pt_params.shard_index and of mi355pt_adaptive.h), and spp_beauty must be 0.
 *   n must be even and >= 2: checked for spp_beauty, a PRECONDITION for tile counts (the adaptive driver produces no other).
 * Prepass, per pixel and channel:  c = B / n,  c1 = H / (n / 2),  c2 = (B - H) / (n / 2);  in each of the three a non-finite or negative
 *   value becomes 0.  a, the normal n and the BACKGROUND rule are exactly those of mi355pt_denoise.h.
 *     irr, irr1, irr2 = c, c1, c2 / (a + albedo_eps)   (c, c1, c2 without A)
 *     lum(x) = ((x.r + x.g) + x.b) / 3
 *     var = ((lum(irr1) - lum(irr2)) / 2)^2              (the variance of the mean of the two half means)
 * Level i = 0 .. levels-1, step s = 2^i, for each non-background pixel p:
 *     sd_p = sqrt(G(var)_p),  G the 3 x 3 binomial filter (1 2 1; 2 4 2; 1 2 1) / 16 over p and its in-frame, non-background neighbours at
 *       distance 1, rows top to bottom and left to right, divided by the sum of the weights it used;
 *   the taps are q = p + s (dx, dy), dx, dy in -2 .. 2; a tap outside the image is skipped, a background tap has weight 0;
 *     d = |lum(irr_p) - lum(irr_q)| / (sigma_lum sd_p + lum_eps) + |n_p - n_q|^2 / sigma_normal^2 + |a_p - a_q|^2 / sigma_albedo^2
 *       (no 4^i factor and no tone curve: the variance does that job)
 *     w = h[dx] h[dy] exp(-d),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *     irr'_p = sum w irr_q / sum w,        var'_p = sum w^2 var_q / (sum w)^2
 *   Background pixels keep their value.  The guides are the same on every level.
 * Output, as mi355pt_denoise.h: irr_final (a + albedo_eps) (irr_final without A) on non-background pixels, c bit for bit on background
 *   pixels: a linear MEAN, i.e. a film with spp = 1 for mi355pt_film_resolve_device.
 *
 * B and H may hold anything (cleaned as above).  The guide films must be FINITE, and c / (a + albedo_eps) and the square of a luminance
 * must not overflow binary32: otherwise the affected pixels and their neighbours are unspecified.
 */
#ifndef MI355PT_DENOISE_VAR_H
#define MI355PT_DENOISE_VAR_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_denoise_var_params {
    uint32_t levels; /* 1 .. 8 */
    float sigma_lum, sigma_normal, sigma_albedo, albedo_eps, lum_eps; /* all finite and > 0 */
} mi355pt_denoise_var_params;

/* levels 5, sigma_lum 4.0, sigma_normal 0.5, sigma_albedo 0.3, albedo_eps 0.01, lum_eps 1e-4 */
void mi355pt_denoise_var_params_default(mi355pt_denoise_var_params* out);
/* Bytes of device scratch mi355pt_denoise_var_device needs for a width x height frame: four 16-byte records per pixel (two irr + variance
 * buffers that ping-pong, the normal + background flag, the albedo).  0 when the product does not fit a size_t. */
size_t mi355pt_denoise_var_scratch_bytes(uint32_t width, uint32_t height);
/* The filter on device buffers.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing, synchronises
 * nothing, uses no atomics and a fixed summation order: two runs are bit-equal.  d_tile_spp (one u32 per 8x8 tile) may be NULL.  d_scratch
 * (16-byte aligned, scratch_bytes >= mi355pt_denoise_var_scratch_bytes) is overwritten.  Returns MI355PT_E_INVALID — before anything
 * touches the device — when: levels is outside 1 .. 8; a sigma, albedo_eps or lum_eps is not finite or not > 0 (a zero-initialised params
 * struct is refused, never interpreted); without tile counts spp_beauty is 0 or odd, with tile counts it is not 0; the spp of a given guide
 * buffer is 0; width or height is 0 (or the frame has more than 2^31 - 1 blocks of 64 x 4 pixels); d_beauty, d_half, d_out, the params
 * pointer or d_scratch is NULL; the scratch is too small or not 16-byte aligned; d_out equals an input pointer (d_tile_spp included). */
int mi355pt_denoise_var_device(const float* d_beauty, const float* d_half, uint32_t spp_beauty, const uint32_t* d_tile_spp,
                               const float* d_albedo, uint32_t spp_albedo, const float* d_normal, uint32_t spp_normal, uint32_t width,
                               uint32_t height, const mi355pt_denoise_var_params* params, void* d_scratch, size_t scratch_bytes,
                               float* d_out, void* hip_stream);
/* The same with host buffers (tile_spp a host array of one u32 per tile, or NULL): allocates the device buffers and the scratch, copies,
 * runs mi355pt_denoise_var_device on the default stream, synchronises and copies the result to `out`.  Same argument checks (scratch
 * aside), before any allocation. */
int mi355pt_denoise_var(const float* beauty, const float* half_film, uint32_t spp_beauty, const uint32_t* tile_spp, const float* albedo,
                        uint32_t spp_albedo, const float* normal, uint32_t spp_normal, uint32_t width, uint32_t height,
                        const mi355pt_denoise_var_params* params, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_DENOISE_VAR_H */
