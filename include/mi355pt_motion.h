/*
 * mi355pt_motion.h — the object-motion block of the C ABI (included by mi355pt.h right after mi355pt_instances.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart.  mi355pt_scene_move_instances (mi355pt_instances.h) moves objects of a built scene; the temporal
 * accumulation (mi355pt_temporal.h, mi355pt_temporal_rectify.h) reprojects a hit with X_prev = X_cur + delta: a static world seen by a
 * moving camera.  This block gives the accumulation OBJECT MOTION VECTORS, so that a frame loop can accumulate across an instance move:
 *
 *   the ID pass        which instance a pixel shows: one primary ray through every pixel centre, a W x H film of u32;
 *   the motion table   where the points of each instance were one frame ago: one affine record per instance, plus a static one (host);
 *   the motion-aware   twins of mi355pt_temporal_accumulate[_device] and mi355pt_temporal_accumulate_rectified[_device] that carry a
 *   accumulation       pixel's hit through its instance's record instead of adding delta, and can hold the taps to the pixel's id.
 *
 * The text below is normative: tests/motion_reference.py restates it in NumPy on top of tests/temporal_reference.py.
 *
 * THE ID PASS.  Per pixel p = (x, y) of the launch's shard (8 x 8 tiles dealt out by params->shard_index / shard_count like the G-buffer
 * pass; a pixel outside the shard is not written): the ray camera.sample_ray(p, uv = (0.5, 0.5)) — the pixel CENTRE, no sampler —, from the
 * render-space origin, not moved forward, closest hit.  ids[p] = (instance of the hit triangle, the index mi355pt_scene_add_instance
 * returned) + 1, or 0 when the ray leaves the scene.  The result does not depend on params->spp, seed or sampler.
 *
 * THE MOTION TABLE.  n + 1 records for a scene of n instances; record i + 1 belongs to instance i — the value the ID pass writes — and
 * record 0 to everything static (a miss never reaches it: a pixel without a hit has no history).  A record takes a render-space point of
 * the CURRENT frame to the render space of the PREVIOUS frame,  X_prev = a X_cur + b,  and a normal likewise,  nrm_prev = n nrm_cur.
 * With the world-space motion  T = l2w_prev l2w_cur^-1  of the instance and the camera positions c_cur, c_prev:
 *     a = lin(T);   b = a c_cur + trans(T) - c_prev;   n = (a^-1)^T.
 * Record 0 is  a = n = I,  b = c_cur - c_prev:  the delta of mi355pt_temporal_view, with the same bits.  An instance whose two matrices
 * are BYTEWISE equal gets record 0's values exactly; no inverse is taken for it.  Everything is computed in double from the f32 inputs
 * and each entry rounded once to f32.
 * n is NOT renormalised (neither is nrm in mi355pt_temporal.h): a motion that changes an object's scale between the two frames changes
 * the length of its normal and so shifts the plane test and the normal test by that factor.  Rigid motions — rotation, translation — are exact.
 *
 * THE MOTION-AWARE ACCUMULATION is the text of mi355pt_temporal.h (and mi355pt_temporal_rectify.h, which builds on its gather) with
 * exactly these changes, for a pixel p:
 *     e = min(ids_cur[p], n_entries - 1);   M = table[e].
 *     Xp_i = ((M.a[3i] X.x + M.a[3i+1] X.y) + M.a[3i+2] X.z) + M.b[i],  i = 0, 1, 2,  replaces  Xp = X + delta;  view->delta is NOT read.
 *     nrm' = the vector ((M.n[3i] nrm.x + M.n[3i+1] nrm.y) + M.n[3i+2] nrm.z)  replaces nrm in the plane test and in the normal test of
 *         the taps: both tests run in the previous frame's render space.
 *     With ids_prev given, a tap q is additionally VALID only if ids_prev[q] == ids_cur[p] (the unclamped value).
 * Every operation is a separate binary32 operation, no fused multiply-add; the loads of all taps — the id taps included — are
 * unconditional, at indices clamped to the frame; no atomics.  With a table of static records and without ids_prev the outputs are
 * bit-equal to those of the existing call (1 x + 0 y + 0 z is x for every finite x, up to the sign of a zero that no output can see).
 */
#ifndef MI355PT_MOTION_H
#define MI355PT_MOTION_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_motion_xform {   /* 96 bytes, 16-byte aligned records on the device */
    float a[9];   /* row-major: X_prev_render = a * X_cur_render + b */
    float b[3];
    float n[9];   /* row-major: nrm_prev = n * nrm_cur (inverse transpose of a) */
    float pad[3];
} mi355pt_motion_xform;

/* The ID pass on a device buffer of W x H u32: ONE launch, asynchronous on `hip_stream` like mi355pt_render_gbuffer_accum_device, with
 * whose argument checks it shares what applies: MI355PT_E_INVALID for a null scene, camera, params or d_ids, a zero-sized frame,
 * collect_stats != 0 and whatever mi355pt_render_aov_accum_device refuses in (scene, camera, params); MI355PT_E_NOT_BUILT for an unbuilt
 * scene.  stats (NULL ok): kernel_ms, launches, samples = closest_rays = the pixels traced, closest_hits. */
int mi355pt_render_ids_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* params, uint32_t* d_ids /* W*H */,
                              void* hip_stream, mi355pt_stats* stats);
/* The same into a host buffer: a zeroed device buffer, the launch on the default stream, the copy back (a pixel outside the shard reads 0). */
int mi355pt_render_ids(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* params, uint32_t* ids /* W*H */,
                       mi355pt_stats* stats);

/* The motion table of a frame pair.  Host only, no device needed.  l2w_cur / l2w_prev: the local_to_world matrices (column-major 4x4, as
 * mi355pt_scene_add_instance takes them) of the n instances in the current and in the previous frame; only the positions of the two
 * cameras are read.  Returns MI355PT_E_INVALID for a null pointer, n == 0, or a non-finite or singular matrix (the lowering's own test:
 * a determinant of the linear part that is exactly zero in double, or an inverse that is not finite) — also of an instance that did not
 * move.  Nothing is written then. */
int mi355pt_motion_table(const mi355pt_camera* cur_cam, const mi355pt_camera* prev_cam, const float* l2w_cur /* n x 16 */,
                         const float* l2w_prev /* n x 16 */, uint32_t n, mi355pt_motion_xform* out /* n + 1 entries */);

/* The motion-aware accumulation on device buffers: the arguments, the launches and every refusal of mi355pt_temporal_accumulate_device,
 * plus d_ids_cur (W x H u32 of the current frame), d_ids_prev (of the previous frame; NULL: no id test of the taps) and d_table
 * (n_entries records, 16-byte aligned).  Without a previous frame (prev == NULL, view == NULL) this IS the existing call: the ids and the
 * table are checked and not read.  Also refused with MI355PT_E_INVALID, before anything touches the device: a NULL d_ids_cur or d_table,
 * n_entries == 0, a d_table that is not 16-byte aligned, an id pointer or the table equal to an output pointer. */
int mi355pt_temporal_accumulate_motion_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                              const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                              const mi355pt_temporal_params* params, const uint32_t* d_ids_cur, const uint32_t* d_ids_prev,
                                              const mi355pt_motion_xform* d_table, uint32_t n_entries, float* d_out_film, float* d_out_half,
                                              float* d_out_length, void* hip_stream);
/* The same with host buffers (ids, table and films), as mi355pt_temporal_accumulate; the table needs no alignment here. */
int mi355pt_temporal_accumulate_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                       const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                       const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_motion_xform* table, uint32_t n_entries,
                                       float* out_film, float* out_half, float* out_length);
/* The rectified form: the arguments and refusals of mi355pt_temporal_accumulate_rectified_device plus the four above; the scratch must
 * not be an id buffer or the table either. */
int mi355pt_temporal_accumulate_rectified_motion_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                        const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                                        const mi355pt_temporal_params* params, const mi355pt_temporal_rectify_params* rectify_params,
                                                        void* d_scratch, size_t scratch_bytes, const uint32_t* d_ids_cur, const uint32_t* d_ids_prev,
                                                        const mi355pt_motion_xform* d_table, uint32_t n_entries, float* d_out_film, float* d_out_half,
                                                        float* d_out_length, void* hip_stream);
int mi355pt_temporal_accumulate_rectified_motion(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                 const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                                 const mi355pt_temporal_rectify_params* rectify_params, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                                 const mi355pt_motion_xform* table, uint32_t n_entries, float* out_film, float* out_half,
                                                 float* out_length);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_MOTION_H */
