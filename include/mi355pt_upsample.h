/*
 * mi355pt_upsample.h — the guided half-resolution block of the C ABI (included by mi355pt.h right after mi355pt_temporal_rectify.h: a caller
 * of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: a joint-bilateral upsample (Kopf et al., SIGGRAPH 2007) of a film traced at W/2 x H/2 to W x H,
 * guided by the G-buffers of mi355pt_gbuffer.h at BOTH resolutions.  The path kernels then trace a quarter of the paths; the full-resolution
 * G-buffer costs a few percent of them.  Each full pixel gathers the 2 x 2 bilinear footprint of low pixels around it, and a low pixel takes
 * part only where it saw the same surface as the full pixel: the tap tests of mi355pt_temporal.h (plane distance in units of the hit
 * distance, shading-normal cosine) and one on the hit film's emitter share.  Optionally the low film is divided by the low albedo and the
 * result multiplied by the full albedo, so that texture detail comes back at full resolution.
 *
 * The text below is normative: tests/upsample_reference.py restates it in NumPy.  All arithmetic is binary32, every operation rounded on
 * its own (no fused multiply-add, no transcendental function, IEEE division), no atomics and a fixed summation order: two runs are
 * bit-equal, and the device result is bit-equal to the restatement.
 *
 * Sizes.  The FULL frame is W x H, both even; the LOW frame is w x h = W/2 x H/2, and low pixel (X, Y) covers the full pixels
 * (2X .. 2X+1, 2Y .. 2Y+1).  Buffers are row-major, y down, W x H x 3 (or w x h x 3) f32.  mi355pt_upsample_low_camera gives the camera of
 * the low frame: the same camera with width and height halved (the aspect ratio is preserved exactly, the vertical fov is the same), so
 * that low pixel (X, Y) sees the union of its four full pixels.  Rendering with it on a scene built for the full camera is allowed: a
 * build fixes the camera's position only.
 *
 * Inputs.  The low film SUMS B of `spp` samples and, optionally, the low half-film SUMS H of its first spp / 2; the LOW and the FULL guides:
 * the raw G-buffer SUMS of mi355pt_gbuffer.h at the two resolutions (any sample counts).  position, shading_normal and hit are required on
 * both sides; albedo is given on both sides or on neither, with its sample counts spp_albedo_low and spp_albedo_full.
 *
 * Per full pixel p = (x, y):
 *   Parent and footprint.  X = x >> 1, Y = y >> 1.   x even: x0 = X - 1, wx = 0.75;  x odd: x0 = X, wx = 0.25;  y0, wy likewise from y.
 *     Taps  q_0 .. q_3 = (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1)  with the bilinear weights  b_0 .. b_3 = (1-wx)(1-wy), wx (1-wy),
 *     (1-wx) wy, wx wy  (9/16, 3/16, 3/16, 1/16 in some order: exact in binary32; the parent (X, Y) is the tap with 9/16).
 *   Tap values.  With a half film:  c1 = clean(H / (spp / 2)),  c2 = clean((B - H) / (spp / 2))  per channel; without:  c = clean(B / spp).
 *     clean is the rule of mi355pt_denoise_var.h: a non-finite or negative value becomes 0.  Everything below that is said of c, i and m
 *     holds for c1, i1, m1 and for c2, i2, m2 alike.
 *   Full-resolution geometry.  hp = hit.y.  hp > 0: a SURFACE pixel with  Xp = position / hp per component,  nrm = 2 (shading_normal / hp) - 1
 *     per component, NOT renormalised,  t = hit.x / hp,  em = hit.z / hp.   hp == 0: a BACKGROUND pixel.
 *     a_p = max(albedo / spp_albedo_full, 0) per channel.
 *   A tap q is VALID iff it lies in the low frame and, with hq = hit_low.y[q],
 *       on a surface pixel      hq > 0;
 *                               |((e.x nrm.x + e.y nrm.y) + e.z nrm.z)| <= pos_tol t,   e = Xp - position_low[q] / hq;
 *                               ((nrm.x nq.x + nrm.y nq.y) + nrm.z nq.z) >= normal_cos,   nq = 2 (shading_normal_low[q] / hq) - 1;
 *                               |em - hit_low.z[q] / hq| <= emitter_tol;
 *       on a background pixel   hq == 0.
 *     (A NaN fails every comparison.)
 *   Value of a valid tap.  On a surface pixel with albedo  i_q = c_q / (a_q + albedo_eps)  per channel,
 *     a_q = max(albedo_low[q] / spp_albedo_low, 0);  otherwise  i_q = c_q.   A valid tap has the weight w_k = b_k; an invalid tap has the
 *     weight 0 AND the value 0, whatever the buffers hold there.
 *   Wt = ((w_0 + w_1) + w_2) + w_3.
 *   Wt > min_weight:   i = (((w_0 i_0 + w_1 i_1) + w_2 i_2) + w_3 i_3) / Wt;   m = i (a_p + albedo_eps) on a surface pixel with albedo,
 *     m = i otherwise.
 *   Otherwise (FALLBACK):  m = c of the parent tap (X, Y), which is always in the low frame.  No demodulation.
 *   Outputs, of the shape of mi355pt_temporal.h's.  With a half film  out_half = m1,  out_film = m1 + m2: a film pair with spp = 2 in the
 *     convention "F = all, H = first half", which mi355pt_denoise_var_device(out_film, out_half, 2, ...), mi355pt_temporal_accumulate_device
 *     and mi355pt_temporal_accumulate_rectified_device (as the current frame, spp 2) and mi355pt_film_resolve_device(out_film, .., 2, ..) take
 *     as it is.  Without  out_film = m: a linear MEAN, spp = 1.   Every pixel of every output is written.
 *
 * Preconditions: the guide films are FINITE.  B and H may hold anything (cleaned as above).
 *
 * Scope: the factor is 2; neighbouring full pixels share taps, so their noise is correlated (a filter that follows does not know that);
 * what a glossy surface reflects is interpolated by the geometry of the surface, not of the reflection.
 */
#ifndef MI355PT_UPSAMPLE_H
#define MI355PT_UPSAMPLE_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_upsample_params {
    float pos_tol, normal_cos, emitter_tol, min_weight, albedo_eps;
} mi355pt_upsample_params;

/* the raw G-buffer sums of one resolution: device pointers for the _device entry point, host pointers for mi355pt_upsample */
typedef struct mi355pt_upsample_guides {
    const float *albedo, *shading_normal, *position, *hit; /* albedo: NULL ok (then on both sides); the others required */
} mi355pt_upsample_guides;

/* pos_tol 0.01, normal_cos 0.9, emitter_tol 0.25, min_weight 0.01, albedo_eps 0.01 */
void mi355pt_upsample_params_default(mi355pt_upsample_params* out);
/* The camera of the low frame: *full with width / 2 and height / 2.  Host only, no device needed.  Returns MI355PT_E_INVALID for a NULL
 * pointer and for a zero or odd width or height. */
int mi355pt_upsample_low_camera(const mi355pt_camera* full, mi355pt_camera* low);
/* The upsample on device buffers: ONE launch.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing,
 * synchronises nothing.  width and height are the FULL size; d_low_film, d_low_half and the low guides are (width / 2) x (height / 2).
 * d_low_half may be NULL (no half film); d_out_half is NULL iff d_low_half is.
 * Returns MI355PT_E_INVALID — before anything touches the device — when: params, d_low_film, d_out_film, low_guides, full_guides or a
 * required guide film (shading_normal, position, hit) is NULL; albedo is given on one side only, or given with spp_albedo_low or
 * spp_albedo_full 0; d_low_half and d_out_half are not both NULL or both given; spp is 0, or odd with a half film; width or height is 0,
 * odd or above 2^24, or the frame has more than 2^31 - 1 blocks of 64 x 4 pixels; pos_tol, emitter_tol, min_weight or albedo_eps is not
 * finite; pos_tol, min_weight or albedo_eps is not > 0; emitter_tol < 0; normal_cos is not in [-1, 1] (a zero-initialised params struct is
 * refused, never interpreted); an output pointer equals an input pointer or the other output. */
int mi355pt_upsample_device(const float* d_low_film, const float* d_low_half, uint32_t spp, const mi355pt_upsample_guides* low_guides,
                            uint32_t spp_albedo_low, const mi355pt_upsample_guides* full_guides, uint32_t spp_albedo_full, uint32_t width,
                            uint32_t height, const mi355pt_upsample_params* params, float* d_out_film, float* d_out_half, void* hip_stream);
/* The same with host buffers: allocates the device buffers, copies, runs mi355pt_upsample_device on the default stream, synchronises and
 * copies the outputs back.  Same argument checks, before any allocation. */
int mi355pt_upsample(const float* low_film, const float* low_half, uint32_t spp, const mi355pt_upsample_guides* low_guides, uint32_t spp_albedo_low,
                     const mi355pt_upsample_guides* full_guides, uint32_t spp_albedo_full, uint32_t width, uint32_t height,
                     const mi355pt_upsample_params* params, float* out_film, float* out_half);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_UPSAMPLE_H */
