/*
 * mi355pt_display.h — the display block of the C ABI (included by mi355pt.h right after mi355pt_upsample.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: what stands between a finished linear film and the picture.  Two operations on device buffers:
 *   METER    a pseudo-logarithmic luminance histogram of the frame, trimmed at both ends, whose mean bin gives an exposure E (a histogram
 *            auto-exposure), blended with the previous frame's; and
 *   DISPLAY  out = encode(tone(clean(F / spp) * E)) with a choice of rational tone curves.
 * mi355pt_params.exposure, which the path kernels multiply into every sample, and mi355pt_film_resolve_device stay what they are; with
 * MI355PT_TONE_REINHARD, MI355PT_ENCODE_SRGB, no record and exposure 1 the display IS that resolve, bit for bit, on a finite non-negative film.
 *
 * The text below is normative: tests/display_reference.py restates it in NumPy.  Every arithmetic step is ONE binary32 operation rounded on
 * its own (no fused multiply-add, IEEE division, no transcendental function — the sole exception is the sRGB OETF of MI355PT_ENCODE_SRGB, the
 * device function mi355pt_film_resolve_device has) or an integer operation; there are no float atomics and no global atomics, and integer
 * counts do not depend on the order they are taken in: two runs are bit-equal, and the meter's record and histogram and the display's
 * MI355PT_ENCODE_LINEAR output are bit-equal to the restatement.  bits(x) is the IEEE bit pattern of a binary32 x as a u32.
 *
 * The film F is W x H x 3 f32 SUMS of `spp` samples, row-major: any film the pipeline produces — a raw accumulation, the spp-2 pairs of
 * mi355pt_temporal.h and mi355pt_upsample.h, a denoiser's output (spp 1).  It may hold anything:  c = clean(F / spp)  per channel, with the
 * clean of mi355pt_denoise_var.h: the quotient where it is > 0 and finite, +0 otherwise.
 *
 * ---- METER (mi355pt_display_meter_device) ----
 * Per pixel.  Y = ((0.2126f c.r + 0.7152f c.g) + 0.0722f c.b)  (three products, two sums; Y >= +0, possibly +inf).
 * Histogram.  256 bins: 32 octaves of 8 bins, the first edge at 2^log2_lum_min.  base = (log2_lum_min + 127) << 3  (= bits(2^log2_lum_min)
 *   >> 20) and t = bits(Y) >> 20.   t < base: the pixel is counted in `below` (zeros, subnormals, cleaned values, everything under
 *   2^log2_lum_min);   t >= base + 256: in `above` (Y >= 2^(log2_lum_min + 32), +inf with it);   otherwise in bin  t - base.  Within an octave
 *   the 8 bins are the top 3 bits of the mantissa: equal WIDTH, not equal ratio — hence pseudo-logarithmic.  Counts are u32.
 * Finish, integers in u64.   N = sum n_k over the 256 bins (below and above are outside it).
 *   cut_lo = (N trim_low) >> 10,  cut_hi = (N trim_high) >> 10.   cut_lo pixels are removed from the bins in ascending order of k — a bin
 *   gives what it has, the last one touched possibly a part —, then cut_hi from what is left in descending order: n'_k.
 *   N' = sum n'_k  (N' >= 1 whenever N >= 1, since trim_low + trim_high < 1024),  S = sum n'_k k  (S <= 2^40).
 *   N' > 0:   pos = (S << 20) / N'  (integer division);   L_avg = the float whose bits are  (base << 20) + pos + (1 << 19): the centre of the
 *             mean bin on the pseudo-log scale;   q = key / L_avg;   E_t = min(max(q, e_min), e_max).
 *   N' == 0:  L_avg = +0;   E_t = word 0 (E) of the previous record when one is given, 1 otherwise.
 *   Adaptation.  With no previous record, or with adapt == 1:  E = E_t EXACTLY (the branch is taken, nothing is computed).  Otherwise, with
 *             E_prev = word 0 of the previous record:   d = E_t - E_prev;  m = d adapt;  E = E_prev + m.   `adapt` in [0, 1] is the caller's:
 *             a caller with a time step dt and a time constant tau passes 1 - exp(-dt / tau), computed on the host.
 * Outputs.  The RECORD, 8 words of 32 bits:  { E, E_t, L_avg (f32);  N, below, above, N' (u32);  0 }.  When d_hist is given, also the 258 u32 of
 *   the histogram BEFORE the trims: the 256 bins, then below, then above.   The previous record is read before the record is written:
 *   d_prev_record may be d_record itself (the usual loop: one record, metered in place frame after frame).
 *   A previous record is a record this function wrote (E finite and > 0).
 * Scaling.  Multiplying the film by 2^j moves every pixel by exactly 8 j bins, so L_avg is multiplied by exactly 2^j and an unclamped E_t by
 *   exactly 2^-j — as long as no pixel enters or leaves the range, nothing becomes subnormal and nothing overflows.
 * Launches: two.  The first reads the film once (12 B per pixel), each block counting into a histogram in LDS (integer LDS adds; a wave whose
 *   lanes share one bin adds its count once) and storing its 258 partial counts as one row of the scratch buffer; the second, one block, sums
 *   the rows in a fixed order of integer additions, finishes and writes the record.  Every word of the scratch that is read has been written
 *   by the first launch: the caller clears nothing.  mi355pt_display_scratch_bytes gives the size, rows x 258 x 4 bytes.
 *
 * ---- DISPLAY (mi355pt_display_device) ----
 * E = word 0 of the record when d_record is given, params.exposure otherwise.  Per channel  x = min(c E, 2^32)  (the cap keeps every curve
 * below free of inf / inf; no curve tells values above it apart), then by params.tone:
 *   MI355PT_TONE_NONE          v = min(x, 1)
 *   MI355PT_TONE_REINHARD      v = x / (1 + x)                                                                 (the curve of the resolve)
 *   MI355PT_TONE_REINHARD_EXT  on the pixel's luminance  Y = ((0.2126f x.r + 0.7152f x.g) + 0.0722f x.b):   w2 = white white (host, f32);
 *                              a = Y / w2;  b = 1 + a;  n = Y b;  d = 1 + Y;  Y' = n / d;  s = Y' / Y;  v = x s  per channel;  Y == 0: v = 0.
 *                              (Luminances at `white` map to 1; a channel may exceed 1: a saturated colour keeps its hue.)
 *   MI355PT_TONE_ACES          Narkowicz's fit:  n = x (2.51f x + 0.03f);  d = x (2.43f x + 0.59f) + 0.14f  (product, sum, product[, sum]);
 *                              v = min(max(n / d, 0), 1)
 *   MI355PT_TONE_HABLE         the Uncharted-2 curve  (x (A x + C B) + D E) / (x (A x + B) + D F) - E / F  with A 0.15, B 0.5, C 0.1, D 0.2,
 *                              E 0.02, F 0.3, taken over its common denominator, where the constant terms cancel (as written, the
 *                              subtraction loses every digit near 0):   p = 0.15f x;   n = x (0.056f p + 0.001f);
 *                              d = 0.06f (x (p + 0.5f) + 0.06f);   h(x) = n / d   (h(0) = 0 exactly; 0.056 = D F - D E, 0.001 = D F C B - D E B).
 *                              v = h(x) / h(white),  h(white) computed once on the host in f32 by the same steps.
 * and by params.encode:  MI355PT_ENCODE_LINEAR stores v;  MI355PT_ENCODE_SRGB stores srgb_oetf(v), the device function of the resolve
 * (12.92 v up to 0.0031308, 1.055 v^(1/2.4) - 0.055 above).   Every value of the output (W x H x 3 f32) is written; one launch.
 *
 * `white` is used by REINHARD_EXT and HABLE and checked always, like every field: a params struct is valid or refused as a whole, by both
 * operations.
 */
#ifndef MI355PT_DISPLAY_H
#define MI355PT_DISPLAY_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MI355PT_TONE_NONE = 0, MI355PT_TONE_REINHARD = 1, MI355PT_TONE_REINHARD_EXT = 2, MI355PT_TONE_ACES = 3, MI355PT_TONE_HABLE = 4 };
enum { MI355PT_ENCODE_LINEAR = 0, MI355PT_ENCODE_SRGB = 1 };
#define MI355PT_DISPLAY_RECORD_WORDS 8
#define MI355PT_DISPLAY_HIST_WORDS 258

typedef struct mi355pt_display_params {
    uint32_t tone, encode;       /* MI355PT_TONE_*, MI355PT_ENCODE_* */
    float exposure;              /* E of the display when no record is given */
    float white;                 /* REINHARD_EXT: the luminance that maps to 1; HABLE: the value that maps to 1 */
    int32_t log2_lum_min;        /* the first bin edge is 2^log2_lum_min */
    uint32_t trim_low, trim_high; /* 1/1024ths of the counted pixels left out at the dark and at the bright end */
    float key, e_min, e_max, adapt;
} mi355pt_display_params;

/* tone REINHARD, encode SRGB, exposure 1, white 11.2, log2_lum_min -16, trim_low 102, trim_high 51, key 0.18, e_min 2^-10, e_max 2^10, adapt 1 */
void mi355pt_display_params_default(mi355pt_display_params* out);
/* Bytes of the meter's scratch buffer for a width x height frame; 0 for a frame the meter refuses.  Host only. */
size_t mi355pt_display_scratch_bytes(uint32_t width, uint32_t height);
/* The meter on device buffers: two launches.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream); allocates nothing,
 * synchronises nothing.  d_record: 8 words; d_prev_record: 8 words, NULL = no previous record, may equal d_record; d_hist: 258 words, NULL =
 * not wanted; d_scratch: scratch_bytes >= mi355pt_display_scratch_bytes(width, height).
 * Returns MI355PT_E_INVALID — before anything touches the device — when: params, d_film, d_scratch or d_record is NULL; spp is 0; width or
 * height is 0 or above 2^24, or the frame has 2^32 pixels or more; scratch_bytes is too small; d_scratch, d_record, d_prev_record or d_hist is
 * not 4-byte aligned; a field of params is refused (below); d_record or d_hist overlaps the film or the scratch buffer, d_hist overlaps
 * d_record or d_prev_record, d_prev_record overlaps the film or the scratch buffer, or d_prev_record overlaps d_record without being it.
 * params is refused — by the meter and by the display alike, a zero-initialised struct with it, never interpreted — when: tone is above
 * MI355PT_TONE_HABLE or encode above MI355PT_ENCODE_SRGB; exposure is not finite or not > 0; white is not finite or outside [2^-16, 2^16];
 * log2_lum_min is outside [-126, 95] (every bin edge, 2^(log2_lum_min + 32) with them, is then a normal float); trim_low + trim_high >= 1024;
 * key, e_min or e_max is not finite or not > 0; e_min > e_max; adapt is not in [0, 1]. */
int mi355pt_display_meter_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* params,
                                 const uint32_t* d_prev_record, void* d_scratch, size_t scratch_bytes, uint32_t* d_record, uint32_t* d_hist,
                                 void* hip_stream);
/* The display on device buffers: ONE launch, asynchronous on `hip_stream`; allocates nothing, synchronises nothing.  d_record NULL: E is
 * params->exposure.
 * Returns MI355PT_E_INVALID — before anything touches the device — when: params, d_film or d_out is NULL; spp is 0; width or height is 0 or
 * above 2^24, or the frame has 2^32 pixels or more; d_record is not 4-byte aligned; a field of params is refused (above); d_out overlaps the
 * film or the record. */
int mi355pt_display_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* params,
                           const uint32_t* d_record, float* d_out, void* hip_stream);
/* The same with host buffers: allocate the device buffers, copy, run the device form on the default stream, synchronise and copy back.  Same
 * argument checks, before any allocation.  prev_record (8 words) and hist (258 words) may be NULL; prev_record may be record. */
int mi355pt_display_meter(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* params,
                          const uint32_t* prev_record, uint32_t* record, uint32_t* hist);
int mi355pt_display(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* params, const uint32_t* record,
                    float* out);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_DISPLAY_H */
