/*
 * mi355pt_bloom.h — the bloom block of the C ABI (included by mi355pt.h right after mi355pt_edit.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the glare of an HDR display chain, between the exposure and the tone curve.  A bright pass over the
 * linear film, a pyramid of [1 3 3 1] reductions, a bilinear expansion back up that mixes every level in, and a composite with the film:
 *     out = clean(F / spp) base + bloom(F) intensity,
 * a W x H x 3 film of spp 1 in unexposed scene units, which mi355pt_display_meter_device, mi355pt_display_device and
 * mi355pt_film_resolve_device take as it is.  An energy-conserving bloom is base = 1 - intensity with threshold 0 (the defaults); the classic
 * additive bloom is base = 1 with a threshold > 0.
 *
 * The text below is normative: tests/bloom_reference.py restates it in NumPy.  Every arithmetic step is ONE binary32 operation rounded on its
 * own (no fused multiply-add), divisions are IEEE, there is no transcendental function and no atomic operation, every sum is taken in the
 * order written: two runs are bit-equal, and every value of the output and of the scratch buffer is bit-equal to the restatement.  min and
 * max are IEEE minNum / maxNum (a NaN operand is ignored).
 *
 * Input.  The film F is W x H x 3 f32 SUMS of `spp` samples, row-major, and may hold anything:  c = clean(F / spp)  per channel, with the
 *   clean of mi355pt_denoise_var.h (the quotient where it is > 0 and finite, +0 otherwise), and  cc = min(c, 2^32).
 * Level sizes.  W_0 = W, H_0 = H;  W_l = (W_{l-1} + 1) >> 1, H_l likewise, for l = 1 .. L = params.levels.  A size that has reached 1 stays 1:
 *   no frame is refused for being small.
 * Bright pass, per pixel of level 0.   m = max(max(cc.r, cc.g), cc.b).   E = word 0 of the display record (mi355pt_display.h) when d_record
 *   is given, params.exposure otherwise.   T = threshold / E;   k = T knee.   a = m - T;   s = min(max(a + k, 0), k + k);
 *   q = (s s) / (4 k), and q = 0 when k == 0;   g = max(q, a);   f = g / m, and f = 0 when m == 0;   p = cc f  per channel.
 *   (The soft knee: nothing below T - k, the quadratic up to T + k, m - T above.  With threshold == 0: T = k = s = q = 0, g = m, f = m / m = 1
 *   and p = cc exactly, with no branch of its own.)
 * Firefly weights (params.firefly == 1; from level 0 to level 1 only).   Y = ((0.2126f p.r + 0.7152f p.g) + 0.0722f p.b);   y1 = 1 + Y;
 *   w = 1 / y1;   the four planes (p.r w, p.g w, p.b w, w) are reduced as below and  D_1 = R(p w) / R(w)  per channel  (R(w) > 0 always, since
 *   Y <= 2^32).  With firefly == 0:  D_1 = R(p).
 * Reduce.  R(S) from level l to level l + 1 is the separable [1 3 3 1] / 8.  Destination (i, j) reads the source columns
 *   x_a = clamp(2 i - 1 + a, 0, W_l - 1), a = 0 .. 3:   per source row  h = (s[x_0] + s[x_3]) + 3 (s[x_1] + s[x_2]);   over the source rows
 *   y_b = clamp(2 j - 1 + b, 0, H_l - 1), b = 0 .. 3:   v = (h[y_0] + h[y_3]) + 3 (h[y_1] + h[y_2]);   R = v (1 / 64).   D_{l+1} = R(D_l).
 * Expand.  X(U) from level l + 1 to the size of level l is bilinear with aligned centres.  For the destination column x:  i = x >> 1;  the
 *   neighbour is n = i + 1 when x is odd, i - 1 otherwise; both clamped to [0, W_{l+1} - 1].   e = 3 u[i] + u[n]  along x (on the rows j and
 *   nj, found from y the same way), then  r = 3 e[j] + e[nj];   X = r (1 / 16).
 * Up pass.  U_L = D_L.  For l = L - 1 .. 1:   U_l = (D_l s0) + (X(U_{l+1}) s1)   with s1 = params.scatter and s0 = 1 - scatter, computed once on
 *   the host in f32.
 * Composite.  B = X(U_1) at W x H;   out = (c base) + (B intensity)  per channel — c, not cc.
 *
 * Scratch buffer (normative, so that a caller can read the levels).  Level l = 1 .. L follows level l - 1; a level is W_l x H_l records of
 * 16 bytes { r, g, b, 0 }, row-major, word 3 written as +0.  The up pass writes U_l over D_l: after the call the buffer holds
 * U_1 .. U_{L-1}, D_L — so a call with levels = l leaves D_l in its place.  Every word that is read was written by the same call: the caller
 * clears nothing.   mi355pt_bloom_scratch_bytes gives the size, 16 sum_{l = 1 .. L} W_l H_l.
 * Launches: 2 L.  L reductions, each workgroup staging the source texels of its tile once in LDS (for level 0: cleaned, capped, bright-passed
 * and weighted once per texel), then L - 1 expansions with the mix and the composite, one thread per destination pixel.
 */
#ifndef MI355PT_BLOOM_H
#define MI355PT_BLOOM_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355PT_BLOOM_MAX_LEVELS 8

typedef struct mi355pt_bloom_params {
    uint32_t levels, firefly;    /* 1 .. 8 levels; firefly 0 or 1 */
    float threshold, knee;       /* in exposed units: the bright pass starts at threshold / E; knee is a fraction of the threshold */
    float scatter;               /* the share of the coarser level in every step of the up pass */
    float base, intensity;       /* out = c base + B intensity */
    float exposure;              /* E of the bright pass when no record is given */
} mi355pt_bloom_params;

/* levels 6, firefly 1, threshold 0, knee 0.5, scatter 0.7, intensity 0.04, base = 1 - 0.04 (in f32), exposure 1 */
void mi355pt_bloom_params_default(mi355pt_bloom_params* out);
/* Bytes of the scratch buffer for a width x height frame and `levels` levels; 0 for what the call refuses.  Host only. */
size_t mi355pt_bloom_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels);
/* The bloom on device buffers: 2 x levels launches, asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing,
 * synchronises nothing.  d_record: the 8 words of a display record, NULL = E is params->exposure; d_scratch: scratch_bytes >=
 * mi355pt_bloom_scratch_bytes(width, height, params->levels); d_out: W x H x 3 f32, and it MAY be d_film itself (the composite reads and
 * writes only its own pixel).
 * Returns MI355PT_E_INVALID — before anything touches the device — when: params, d_film, d_scratch or d_out is NULL; spp is 0; width or
 * height is 0 or above 2^24, or the frame has 2^32 pixels or more; a field of params is refused (below); scratch_bytes is too small; d_scratch
 * is not 16-byte aligned or d_record not 4-byte aligned; d_out overlaps the film without being it; d_out, the film, the scratch buffer and
 * the record overlap in any other way.
 * params is refused — a zero-initialised struct with it, never interpreted — when: levels is outside [1, 8]; firefly is above 1; threshold is
 * not finite or outside [0, 2^16]; knee, scatter or base is outside [0, 1]; intensity is outside [0, 16]; exposure is not finite or not > 0. */
int mi355pt_bloom_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* params,
                         const uint32_t* d_record, void* d_scratch, size_t scratch_bytes, float* d_out, void* hip_stream);
/* The same with host buffers: allocate the device buffers (the scratch among them), copy, run the device form on the default stream,
 * synchronise and copy back.  Same argument checks, before any allocation.  record (8 words) may be NULL; out may be film. */
int mi355pt_bloom(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* params, const uint32_t* record,
                  float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_BLOOM_H */
