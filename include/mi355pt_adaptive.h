/*
 * mi355pt_adaptive.h — the adaptive-sampling block of the C ABI (included by mi355pt.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference gives every pixel the same --spp.  Here the frame's 8x8 tiles (tile t = (t % tiles_x,
 * t / tiles_x), tiles_x = ceil(W / 8), the tiles of mi355pt_params.shard_index) carry their own sample count, and samples go on where
 * a per-tile noise estimate is above a threshold.  The text below is normative: tests/adaptive_reference.py restates it in NumPy.
 *
 * State of a frame, all device buffers:
 *   F          film: linear sums, W x H x 3 f32, what mi355pt_render_accum_device writes
 *   H          half film, the same layout
 *   tile_spp   one u32 per tile
 *   tile_err   one f32 per tile
 * Invariant the driver keeps: a tile with tile_spp = n holds F = the sum of sample indices [0, n) and H = the sum of [0, n / 2).
 *
 * Noise of a tile with tile_spp = n (n even, n >= 2), in binary32, every operation rounded on its own (no fused multiply-add), in the
 * order written.  Per in-frame pixel and channel c:  m.c = F.c / (float)n,  h.c = H.c / (float)(n / 2);
 *     d   = (|m.r - h.r| + |m.g - h.g|) + |m.b - h.b|
 *     s   = max((m.r + m.g) + m.b, 0) + dark_eps
 *     e_p = d / sqrt(s)                      (division and square root correctly rounded)
 * Per tile: v[l], l = 8 (y & 7) + (x & 7), is e_p of the tile's pixel (x, y) and 0 for a pixel outside the frame; the 64 values are summed
 * as a pairwise tree — for k = 32, 16, 8, 4, 2, 1 in turn: v[l] = v[l] + v[l + k] for every l < k — and
 *     e_t = v[0] / (float)(number of in-frame pixels of the tile).
 * A NaN or an infinity in F or H of an in-frame pixel makes e_t NaN (inf - inf and inf / inf are NaN).
 *
 * Step at level_spp, for every tile with tile_spp == level_spp (tiles at other counts are untouched, in every buffer):
 *     tile_err = e_t;   the tile is ACTIVE when !(e_t <= threshold) and level_spp < max_spp — a NaN error keeps sampling up to the maximum;
 *     an active tile copies H := F on its in-frame pixels and sets tile_spp = 2 level_spp (it now owes the samples [level_spp, 2 level_spp)).
 * The indices of the active tiles go to d_list in ascending order, their number to d_count.
 */
#ifndef MI355PT_ADAPTIVE_H
#define MI355PT_ADAPTIVE_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_adaptive_params {
    float threshold; /* finite and > 0; no default: it is in units of sqrt(radiance) and belongs to the picture */
    float dark_eps;  /* finite and > 0: keeps e_p finite on black pixels; the CLI uses 1e-3 */
    uint32_t min_spp; /* a power of two, >= 2: every tile gets this many samples before the first estimate */
} mi355pt_adaptive_params;

typedef struct mi355pt_adaptive_result {
    uint32_t passes;        /* steps run (the one that found nothing active included) */
    uint32_t tiles_at_max;  /* tiles whose tile_spp is params.spp at the end */
    uint64_t total_samples; /* sum over tiles of tile_spp x in-frame pixels of the tile */
} mi355pt_adaptive_result;

/* Bytes of device scratch mi355pt_adaptive_step_device and the drivers need for a width x height frame: one u32 flag per tile, rounded up
 * to 16, plus 16 (the drivers keep the count there).  0 when the frame is empty or has 2^31 tiles or more. */
size_t mi355pt_adaptive_scratch_bytes(uint32_t width, uint32_t height);
/* The step defined above, on device buffers.  d_list: room for one u32 per tile; d_count: one u32.  Asynchronous on `hip_stream`; allocates
 * nothing, synchronises nothing, uses no float atomics and a fixed summation order: two runs are bit-equal.  Returns MI355PT_E_INVALID —
 * before anything touches the device — when: a pointer is NULL; width or height is 0 (or the frame has 2^31 tiles or more); threshold or
 * dark_eps is not finite or not > 0, or min_spp is not a power of two >= 2 (a zero-initialised params struct is refused, never interpreted);
 * level_spp is odd or 0; max_spp < level_spp; the scratch is smaller than mi355pt_adaptive_scratch_bytes or not 4-byte aligned. */
int mi355pt_adaptive_step_device(const float* d_film, float* d_half, uint32_t width, uint32_t height, uint32_t* d_tile_spp, float* d_tile_err,
                                 const mi355pt_adaptive_params* params, uint32_t level_spp, uint32_t max_spp, void* d_scratch,
                                 size_t scratch_bytes, uint32_t* d_list, uint32_t* d_count, void* hip_stream);
/* d_mean = F / (float)tile_spp of the pixel's tile, per value (W x H x 3 f32; d_mean may be d_film): a linear MEAN, i.e. a film with
 * spp = 1 like the denoiser's output — for mi355pt_film_resolve_device(.., spp = 1, ..) and mi355pt_denoise_device(.., spp_beauty = 1, ..).
 * Asynchronous on `hip_stream`.  MI355PT_E_INVALID on a NULL pointer or an empty / too large frame.  A tile_spp of 0 divides by 0. */
int mi355pt_film_normalize_tiles_device(const float* d_film, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_mean,
                                        void* hip_stream);
/* The driver.  p->spp is the MAXIMUM: a power of two >= adaptive->min_spp; it fixes the Sobol sequence of every range, so a tile's film at
 * count n is what mi355pt_render_accum_device gives for [0, n) with the same params.  p->shard_count must be 0 or 1 and p->collect_stats 0.
 * The sequence is normative (min = adaptive->min_spp, max = p->spp):
 *   1. F = 0, H = 0, tile_spp = min for every tile;
 *   2. the whole frame [0, min / 2) into H (mi355pt_render_accum_device);     3. F := H;
 *   4. the whole frame [min / 2, min) into F;
 *   5. for level = min, 2 min, .. <= max: the step at level; read back the count (4 bytes: the only host round trip of a pass); count 0
 *      ends the loop; otherwise the listed tiles [level, 2 level) into F (the launch of mi355pt_render_accum_tiles_device, the list
 *      staying on the device).
 * The step at level == max activates nothing, so on return every tile's tile_err is the error of its final F and H.
 * Device buffers: d_film, d_half (W x H x 3 f32), d_tile_spp (u32), d_tile_err (f32), d_list (u32) with one entry per tile each, d_scratch
 * (mi355pt_adaptive_scratch_bytes).  Runs on `hip_stream` and synchronises it once per pass.  `result` may be NULL. */
int mi355pt_render_adaptive_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p,
                                   const mi355pt_adaptive_params* adaptive, float* d_film, float* d_half, uint32_t* d_tile_spp,
                                   float* d_tile_err, uint32_t* d_list, void* d_scratch, size_t scratch_bytes, void* hip_stream,
                                   mi355pt_adaptive_result* result);
/* The same with host output: allocates the buffers, runs the driver on the default stream, then mi355pt_film_normalize_tiles_device and
 * mi355pt_film_resolve_device(spp = 1) into out_rgb (host, W*H*3, like mi355pt_render); out_tile_spp (host, one u32 per tile) and `result`
 * may be NULL. */
int mi355pt_render_adaptive(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p,
                            const mi355pt_adaptive_params* adaptive, float* out_rgb, uint32_t* out_tile_spp, mi355pt_adaptive_result* result);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_ADAPTIVE_H */
