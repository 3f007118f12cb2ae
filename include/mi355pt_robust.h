/*
 * mi355pt_robust.h — the robust-film block of the C ABI (included by mi355pt.h right after mi355pt_display.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: firefly rejection by a median of means.  The film is one sum per pixel, so one sample of radiance
 * 10^3 stays in the picture for good.  The n samples of a frame rendered as K BUCKETS of n / K consecutive sample indices give K
 * independent means per pixel; a trimmed mean of those, whose trim is chosen per pixel from the Gini coefficient of the bucket means — none
 * where the buckets agree, the median where one bucket holds a spike — is the estimator of Buisine, Delepoulle and Renaud, "Firefly removal
 * in Monte Carlo rendering with adaptive Median of meaNs" (EGSR 2021).  The estimator is BIASED LOW on right-skewed pixels (DESIGN.md 4.15
 * has the numbers): the block is opt-in, the path kernels and the reference's estimator (mi355pt_render) are untouched.
 *
 * The text below is normative: tests/robust_reference.py restates it in NumPy.  All arithmetic is binary32, every operation rounded on its
 * own (no fused multiply-add, IEEE division); there are no atomics and the order of every sum is fixed: two runs are bit-equal, and every
 * output value is bit-equal to the restatement.
 *
 * Input.  d_buckets holds K row-major W x H x 3 f32 films of linear SUMS, one after another: bucket k starts at float offset k W H 3.  Each
 * bucket is over spp_bucket samples.  The procedure is defined over a SET of N buckets taken in ascending bucket index.
 *
 * Per pixel:
 *   1. Clean the bucket means.  For bucket k and each channel  v = B_k / (float)spp_bucket;  m_k = v if v is finite and v > 0, otherwise +0.
 *   2. Luminance:  l_k = ((m_k.r + m_k.g) + m_k.b) / 3.
 *   3. Rank:  r_k = #{ j != k : l_j < l_k or (l_j == l_k and j < k) }  — a permutation of 0 .. N-1.
 *   4. Sums, accumulated from +0 in bucket order:   S = sum_k l_k;   Q = sum_k (float)(2 r_k - (N - 1)) l_k, each product rounded, then added.
 *   5. Gini term:  G = Q / ((float)(N - 1) S) if S > 0, else 0  (the Gini coefficient normalised so that ONE non-zero bucket gives 1);
 *      g = min(1, max(0, gini_scale G)).
 *   6. Trim count t by params.mode:
 *        MI355PT_ROBUST_GMON   t = min(N/2 - 1, (int)floorf(g (float)(N/2)))
 *        MI355PT_ROBUST_MOM    t = N/2 - 1        (the median of means: the two middle buckets)
 *        MI355PT_ROBUST_MEAN   t = 0
 *   7. Output:  theta = (sum_{k : t <= r_k < N - t} m_k) / (float)(N - 2t)  per channel, the sum in bucket order from +0.
 *
 * Output modes.
 *   Single (d_out_half == NULL): the set is all K buckets, N = K.  d_out = theta, a linear MEAN: a film with spp 1 for
 *     mi355pt_film_resolve_device, mi355pt_denoise_device and the display stage.
 *   Pair (d_out_half != NULL): the even-indexed and the odd-indexed buckets are two sets of N = K/2.  d_out_half = theta_even and
 *     d_out = theta_even + theta_odd (one addition): the film pair with spp 2 that mi355pt_denoise_var_device and
 *     mi355pt_film_resolve_device take as it is.
 *   d_out_trim (NULL ok): two bytes per pixel, (t, 0) for single output and (t_even, t_odd) for pair output.
 *
 * Preconditions.  S and the channel sums must not overflow binary32; a pixel where one does is unspecified.  Buckets may hold NaN, +-inf and
 * negative values: step 1 cleans them.
 *
 * One launch, one thread per pixel; it reads the K films once (12 K bytes per pixel) and writes 12 (24 for a pair, + 2 with the trims) bytes.
 */
#ifndef MI355PT_ROBUST_H
#define MI355PT_ROBUST_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MI355PT_ROBUST_MEAN = 0, MI355PT_ROBUST_MOM = 1, MI355PT_ROBUST_GMON = 2 };

typedef struct mi355pt_robust_params {
    uint32_t mode;               /* MI355PT_ROBUST_* */
    float gini_scale;            /* GMON: the factor on the Gini term before it is clamped to [0, 1] */
} mi355pt_robust_params;

/* mode GMON, gini_scale 1 */
void mi355pt_robust_params_default(mi355pt_robust_params* out);
/* The combination on device buffers: ONE launch, asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing,
 * synchronises nothing; no atomics and a fixed order, so two runs are bit-equal.  d_out and d_out_half: W x H x 3 f32; d_out_trim: W x H x 2
 * bytes.
 * Returns MI355PT_E_INVALID — before anything touches the device — when: params, d_buckets or d_out is NULL; n_buckets is not 4, 8, 16 or 32;
 * spp_bucket is 0; width or height is 0 or above 2^24, or the frame has 2^32 pixels or more; mode is above MI355PT_ROBUST_GMON; gini_scale
 * is not finite or is < 0 (a zero-initialised struct is MEAN with scale 0 and is accepted); two of d_out, d_out_half and d_out_trim are
 * equal or overlap, or one of them lies inside or overlaps the n_buckets x W x H x 3 floats at d_buckets. */
int mi355pt_robust_combine_device(const float* d_buckets, uint32_t n_buckets, uint32_t spp_bucket, uint32_t width, uint32_t height,
                                  const mi355pt_robust_params* params, float* d_out, float* d_out_half, uint8_t* d_out_trim, void* hip_stream);
/* The same with host buffers: allocate the device buffers, copy, run the device form on the default stream, synchronise and copy back.  Same
 * argument checks, before any allocation. */
int mi355pt_robust_combine(const float* buckets, uint32_t n_buckets, uint32_t spp_bucket, uint32_t width, uint32_t height,
                           const mi355pt_robust_params* params, float* out, float* out_half, uint8_t* out_trim);
/* The frame of (scene, cam, p) as n_buckets films: clears the n_buckets x W x H x 3 floats at d_buckets on the stream, then makes n_buckets
 * calls of mi355pt_render_accum_device's path, bucket k over the sample indices [k spp / K, (k + 1) spp / K) into film k.  Each bucket film
 * is what mi355pt_render_accum_device gives for that range on a zeroed film, bit for bit; shard_index and shard_count are honoured (the
 * pixels of other shards stay 0 in every bucket).  The SUM of the buckets is NOT promised to equal the one-launch film of [0, spp) bit for
 * bit: the order of the summation differs.
 * Returns MI355PT_E_INVALID — before anything touches the device — when a pointer but `stats` is NULL, n_buckets is not 4, 8, 16 or 32,
 * p->spp is not a multiple of n_buckets (0 with it) or p->collect_stats != 0; then the checks of mi355pt_render_accum_device.
 * `stats`, when given, receives the summed kernel_ms and launches of the bucket launches (the rest is 0) and synchronises the stream. */
int mi355pt_render_buckets_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t n_buckets, float* d_buckets,
                                  void* hip_stream, mi355pt_stats* stats /* NULL ok; non-NULL synchronises the stream */);
/* The seam's shape (mi355pt_render): mi355pt_render_buckets_device, the single-output combination, mi355pt_film_resolve_device with spp 1;
 * fills out_rgb (host, W*H*3) with tone-mapped sRGB-encoded values.  Allocates, synchronises.  The checks of the three, before any allocation. */
int mi355pt_render_robust(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t n_buckets,
                          const mi355pt_robust_params* robust_params, float* out_rgb);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_ROBUST_H */
