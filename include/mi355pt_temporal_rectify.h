/*
 * mi355pt_temporal_rectify.h — the history-rectification block of the C ABI (included by mi355pt.h right after mi355pt_temporal.h: a caller
 * of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart.  mi355pt_temporal.h blends each frame into a history of up to max_history frames and never asks
 * whether that history still agrees with what the current frame says: after a change of illumination the stale image keeps the weight
 * (1 - 1 / L) per frame.  The accumulation declared here RECTIFIES the gathered history first: over a window around each pixel it compares
 * the MEAN of the current frame with the mean of the gathered history — the signal's own variation cancels between the two — allows the
 * history's mean to differ by gamma standard errors of the current mean, and scales the history by the ratio that brings it back.  (The
 * usual variance clipping to the neighbourhood's colour box is too weak at a few spp: the box of a noisy Monte-Carlo neighbourhood reaches
 * down to 0, so a history that is too dark is never corrected.)
 *
 * The text below is normative: tests/temporal_rectify_reference.py restates it in NumPy.  Everything that mi355pt_temporal.h defines is used
 * unchanged: c (or c1, c2), "has history", hist (or hist1, hist2), L and a = 1 / L.  All arithmetic is binary32, every operation rounded
 * on its own (no fused multiply-add), division and square root are IEEE (correctly rounded), no atomics and a fixed summation order: two
 * runs are bit-equal, and the device result is bit-equal to the restatement.
 *
 * Per pixel p:
 *   v_p = (c1 + c2) 0.5 per channel with a half film, c without.       g_p = (hist1 + hist2) 0.5 with a half film, hist without.
 *   A pixel without history has g = 0 and is not a MEMBER of any window.
 *   Window of p: the in-frame pixels q with |dx|, |dy| <= radius that have a history.
 *   Four sums per channel: S1 = sum v, S2 = sum (v v), Sg = sum g, and the member count n (one value, not per channel).  Each is formed as
 *   ROW sums first — dx = -radius .. radius left to right, starting from 0, a non-member contributing the value 0 — and the row sums are
 *   then added for dy = -radius .. radius top to bottom, starting from 0.
 * For p with history (n >= 1), per channel:
 *   mu = S1 / n;   s2 = S2 / n - mu mu, set to 0 unless s2 > 0;   se = sqrt(s2 / n);   muh = Sg / n;
 *   lo = mu - gamma se;   hi = mu + gamma se;   tgt = min(max(muh, lo), hi);   k = tgt / muh if muh > 0, else 1;
 *   hist' = hist k (hist1 and hist2 take the same k);   m = hist' + (c - hist') a.
 * A pixel without history gets m = c and L = 1, as in mi355pt_temporal.h.  L and out_length are exactly that header's.
 * Outputs, of that header's shape: out_half = m1, out_film = m1 + m2; out_film = m without a half film.
 *
 * Preconditions: the previous films are finite where the previous length is > 0, and no square or window sum overflows binary32; otherwise
 * the affected windows are unspecified.  The current film may hold anything (it is cleaned as in mi355pt_temporal.h).
 */
#ifndef MI355PT_TEMPORAL_RECTIFY_H
#define MI355PT_TEMPORAL_RECTIFY_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_temporal_rectify_params {
    uint32_t radius;      /* the window is (2 radius + 1)^2 pixels: 1 .. 3 */
    float gamma;          /* the history's window mean may differ from the current one by gamma standard errors: finite, > 0 */
} mi355pt_temporal_rectify_params;

/* radius 2, gamma 2.0: the values of the NumPy study that chose the rule (profiles/temporal_rectify_cpu.json), not tuned further */
void mi355pt_temporal_rectify_params_default(mi355pt_temporal_rectify_params* out);
/* 32 bytes per pixel — the gathered history between the two launches; 0 when the product does not fit a size_t */
size_t mi355pt_temporal_rectify_scratch_bytes(uint32_t width, uint32_t height);
/* mi355pt_temporal_accumulate_device with the rectification: TWO launches on `hip_stream` (the gather into d_scratch, the rectifying blend).
 * Asynchronous, allocates nothing, synchronises nothing, no atomics.  With prev == NULL (and view == NULL) it IS that function's first
 * frame, and d_scratch is not touched (it is checked all the same).
 * Returns MI355PT_E_INVALID — before anything touches the device — for everything mi355pt_temporal_accumulate_device refuses, and when:
 * rectify_params is NULL; radius is not 1 .. 3; gamma is not finite or not > 0 (a zero-initialised struct is refused, never interpreted);
 * d_scratch is NULL, not 16-byte aligned, or scratch_bytes < mi355pt_temporal_rectify_scratch_bytes(width, height); d_scratch equals an
 * input or an output pointer. */
int mi355pt_temporal_accumulate_rectified_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                 const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                                 const mi355pt_temporal_params* params, const mi355pt_temporal_rectify_params* rectify_params,
                                                 void* d_scratch, size_t scratch_bytes, float* d_out_film, float* d_out_half, float* d_out_length,
                                                 void* hip_stream);
/* The same with host buffers, as mi355pt_temporal_accumulate: it allocates the device buffers and its own scratch.  Same argument checks
 * (the scratch's aside), before any allocation. */
int mi355pt_temporal_accumulate_rectified(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                          const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                          const mi355pt_temporal_rectify_params* rectify_params, float* out_film, float* out_half, float* out_length);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_TEMPORAL_RECTIFY_H */
