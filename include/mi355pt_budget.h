/*
 * mi355pt_budget.h — the sample-budget block of the C ABI (included by mi355pt.h right after mi355pt_flow.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart.  The temporal accumulation (mi355pt_temporal.h, mi355pt_motion.h, mi355pt_flow.h) restarts a pixel
 * whose reprojection finds no valid tap at history length 1: a DISOCCLUSION shows the frame's few samples beside neighbours that hold 32
 * frames.  This block spends the frame's samples where the history will be missing, BEFORE the frame is rendered:
 *
 *   the history probe   the geometric half of the temporal gather on the G-buffers alone: per pixel the history length the accumulation
 *                       will find, per 8 x 8 tile its minimum and from it a sample count;
 *   the budget driver   renders a frame with those per-tile counts over the tile-list renders (mi355pt_render_accum_tiles_device), keeping
 *                       the adaptive driver's invariant of F and H (mi355pt_adaptive.h);
 *   the pair normalise  turns that F / H pair with per-tile counts into a film pair with spp = 2, which every
 *                       mi355pt_temporal_accumulate* call takes as it is;
 *   the length credit   adds the frames' worth of extra samples to the accumulated length of the boosted tiles.
 *
 * A frame loop: G-buffer (and ids / flow records), probe, driver, pair normalise, the accumulation with spp = 2, length credit.  No path
 * kernel and none of the twelve accumulation calls changes.  The text below is normative: tests/budget_reference.py restates it in NumPy on
 * top of tests/temporal_reference.py, tests/motion_reference.py and tests/flow_reference.py.  All arithmetic is binary32, every operation
 * rounded on its own (no fused multiply-add), no atomics: two runs are bit-equal, and the device result is bit-equal to the restatement.
 * Tiles are those of mi355pt_adaptive.h: tile t = (t % tiles_x, t / tiles_x), tiles_x = ceil(W / 8).
 *
 * THE PROBE.  Per pixel p, with every symbol exactly as in mi355pt_temporal.h — and with Xp and nrm carried as mi355pt_motion.h says when
 * a table is given, or as mi355pt_flow.h says when flow records are given, the previous-id test of the taps included —:
 *     P = Lh   if the pixel has history (none of the "no history" cases, and Wt > min_weight),   P = 0 otherwise.
 * Lh is the gathered length BEFORE the + 1: the accumulation of the same inputs writes out_length = min(P + 1, max_history) where P > 0
 * and 1 elsewhere, bit for bit.  Without a previous frame every P is 0 and no G-buffer is read.  The current frame's position,
 * shading_normal and hit films and the previous frame's length, position, shading_normal and hit films are read; film and half pointers
 * are ignored and never read.  The loads of all taps are unconditional, at indices clamped to the frame.
 * Per tile t:  Lmin = the minimum over the tile's in-frame pixels of P, a P that is not > 0 counting as 0 (so the minimum does not depend
 * on the order);   tile_len[t] = Lmin;   tile_spp[t] = base_spp << j,  j the smallest integer >= 0 with
 *     (Lmin + 1.0f) * 2^j >= target_history   or   base_spp << j == max_spp
 * (Lmin + 1 is rounded once; the scale by a power of two is exact).  A tile whose every pixel will reach target_history frames' worth of
 * samples with this frame's base_spp gets base_spp; a tile with a pixel that starts over gets base_spp * 2^ceil(log2 target_history),
 * capped at max_spp.
 *
 * THE DRIVER.  p->spp must equal max_spp: it fixes the Sobol sequence of every range, so a tile's film at count n is what
 * mi355pt_render_accum_device gives for [0, n) with the same params.  p->shard_count must be 0 or 1 and p->collect_stats 0.  Every
 * tile_spp[t] must be a power of two in [base_spp, max_spp]; a value outside is clamped into the range on the device, never trusted (and a
 * value inside that is no power of two renders as the next power of two).  The sequence is normative (base = base_spp, max = max_spp):
 *   1. F = 0, H = 0;
 *   2. the whole frame [0, base / 2) into H (mi355pt_render_accum_device);     3. F := H;
 *   4. the whole frame [base / 2, base) into F;
 *   5. for level = base, 2 base, .. < max: the tiles with tile_spp > level go to d_list in ascending order; their count is read back (4
 *      bytes: the only host round trip of a pass); a count of 0 ends the loop; otherwise H := F on the listed tiles' in-frame pixels, and
 *      the listed tiles' [level, 2 level) into F (the launch of mi355pt_render_accum_tiles_device, the list staying on the device).
 * On return a tile with count n holds F = the sum of [0, n) and H = the sum of [0, n / 2): the invariant of mi355pt_adaptive.h, which
 * mi355pt_denoise_var_device takes with d_tile_spp.  tile_spp is not written.
 *
 * THE PAIR NORMALISE.  Per value of both films,  out = in / (float)(n_t / 2),  n_t the count of the pixel's tile: a film pair with spp = 2
 * in the convention "F = all, H = first half" (F / (n / 2) = 2 mean, H / (n / 2) = the mean of the first half).  Every
 * mi355pt_temporal_accumulate* call, mi355pt_denoise_var_device and mi355pt_film_resolve_device take it as it is with spp = 2.
 *
 * THE LENGTH CREDIT, in place on the accumulation's out_length: on the pixels of tiles with n_t > base_spp,
 *     length := min(length + (float)(n_t / base_spp - 1), max_history)        (an integer quotient)
 * Tiles at base_spp (or below) are not written.  A disoccluded pixel rendered at 8 base_spp leaves the frame with length 8, so the next
 * frame's blend weighs it as the 8 frames' worth of samples it is.
 *
 * THE KNOWN LIMIT.  The blend weight of the CURRENT frame stays 1 / L whatever the tile's count: a boosted pixel that HAD some history is
 * under-weighted this frame (its n_t / base_spp frames' worth of new samples count as one frame's).  The result is unbiased — every blend is
 * a convex combination of unbiased estimates — but not variance-optimal.  Weighing by the count would take a per-tile-count variant of all
 * twelve gathers and is out of scope.
 */
#ifndef MI355PT_BUDGET_H
#define MI355PT_BUDGET_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_budget_params {
    uint32_t base_spp;       /* power of two >= 2: every tile gets this many samples */
    uint32_t max_spp;        /* power of two >= base_spp */
    float    target_history; /* finite, >= 1: the history length a tile should reach this frame */
} mi355pt_budget_params;

typedef struct mi355pt_budget_motion {   /* how a pixel is carried into the previous frame */
    const uint32_t* ids_cur;             /* mi355pt_motion.h / mi355pt_flow.h */
    const uint32_t* ids_prev;
    const mi355pt_motion_xform* table;   /* table form */
    uint32_t n_entries;
    const mi355pt_flow_pixel* flow;      /* per-pixel form */
} mi355pt_budget_motion;                 /* NULL pointer or all-zero struct: static world (X + delta) */

/* The probe on device buffers: ONE launch.  Asynchronous on `hip_stream`; allocates nothing, synchronises nothing.  prev == NULL (then view
 * must be NULL too) is the first frame.  d_pred_length (W x H f32, NULL ok) receives P; d_tile_len (f32) and d_tile_spp (u32) have one
 * entry per tile.  Returns MI355PT_E_INVALID — before anything touches the device — when: cur, temporal_params, budget_params, d_tile_len
 * or d_tile_spp is NULL; prev and view are not both NULL or both given; cur lacks position, shading_normal or hit, or prev lacks length
 * or one of those three; width or height is 0 (or above 2^24, or the frame has 2^31 tiles or more); the temporal params are what
 * mi355pt_temporal_accumulate_device refuses; base_spp is not a power of two >= 2, max_spp not a power of two >= base_spp, target_history
 * not finite or < 1; motion gives both a table and flow records, or ids without either; the table form or the flow form breaks the pointer
 * rules of mi355pt_temporal_accumulate_motion_device / mi355pt_temporal_accumulate_flow_device (the three outputs here in the place of
 * theirs); an output pointer equals a film that is read or another output.  Without a previous frame the motion is checked and not read. */
int mi355pt_temporal_budget_device(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view,
                                   uint32_t width, uint32_t height, const mi355pt_temporal_params* temporal_params,
                                   const mi355pt_budget_motion* motion, const mi355pt_budget_params* budget_params, float* d_pred_length,
                                   float* d_tile_len, uint32_t* d_tile_spp, void* hip_stream);
/* The same with host buffers (films, ids, table or records, outputs): allocates the device buffers, copies, runs the device form on the
 * default stream and copies the outputs back.  Same argument checks, before any allocation; the table and the records need no alignment. */
int mi355pt_temporal_budget(const mi355pt_temporal_frame* cur, const mi355pt_temporal_frame* prev, const mi355pt_temporal_view* view, uint32_t width,
                            uint32_t height, const mi355pt_temporal_params* temporal_params, const mi355pt_budget_motion* motion,
                            const mi355pt_budget_params* budget_params, float* pred_length, float* tile_len, uint32_t* tile_spp);

/* The driver.  Device buffers: d_tile_spp (in: one u32 per tile), d_film, d_half (W x H x 3 f32), d_list (one u32 per tile), d_scratch
 * (mi355pt_adaptive_scratch_bytes, 4-byte aligned).  Runs on `hip_stream` and synchronises it once per pass of step 5.  `result` (NULL ok):
 * passes = the passes of step 5 that were run (the one that found nothing included), tiles_at_max and total_samples as in mi355pt_adaptive.h,
 * from the clamped counts.  MI355PT_E_INVALID, before anything touches the device: whatever mi355pt_render_accum_tiles_device refuses in
 * (scene, camera, params); budget params as above; p->spp != max_spp; a NULL buffer; a scratch that is missing, too small or misaligned. */
int mi355pt_render_budget_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p,
                                 const mi355pt_budget_params* budget_params, const uint32_t* d_tile_spp, float* d_film, float* d_half,
                                 uint32_t* d_list, void* d_scratch, size_t scratch_bytes, void* hip_stream, mi355pt_adaptive_result* result);

/* The pair normalise on device buffers: ONE launch, asynchronous on `hip_stream`.  In place is allowed: d_out_film == d_film and
 * d_out_half == d_half.  MI355PT_E_INVALID on a NULL pointer, an empty or too large frame (as the probe), d_out_film == d_out_half, or an
 * output that is the OTHER film's input.  A tile_spp of 0 or 1 divides by 0. */
int mi355pt_film_pair_normalize_tiles_device(const float* d_film, const float* d_half, const uint32_t* d_tile_spp, uint32_t width, uint32_t height,
                                             float* d_out_film, float* d_out_half, void* hip_stream);
/* The same with host buffers. */
int mi355pt_film_pair_normalize_tiles(const float* film, const float* half, const uint32_t* tile_spp, uint32_t width, uint32_t height, float* out_film,
                                      float* out_half);

/* The length credit on device buffers, in place: ONE launch, asynchronous on `hip_stream`.  MI355PT_E_INVALID on a NULL pointer, an empty or
 * too large frame, a base_spp that is not a power of two >= 2, a max_history that is not finite or < 1. */
int mi355pt_temporal_length_credit_device(float* d_length, const uint32_t* d_tile_spp, uint32_t base_spp, float max_history, uint32_t width,
                                          uint32_t height, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_BUDGET_H */
