/*
 * mi355pt_flow.h — the per-pixel motion block of the C ABI (included by mi355pt.h right after mi355pt_deform.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart.  A built scene changes in place three ways: mi355pt_scene_move_camera (mi355pt_rebase.h),
 * mi355pt_scene_move_instances (mi355pt_instances.h) and mi355pt_scene_deform_meshes (mi355pt_deform.h).  The temporal accumulation
 * follows the first (mi355pt_temporal.h: X + delta, a static world) and the second (mi355pt_motion.h: one affine record per instance).
 * This block follows all three, and any mix of them, with ONE mechanism: a motion record per PIXEL.  All three moves keep the tree's
 * topology and its leaf order, so triangle i of the leaf-order array is the same triangle of the same mesh before and after a move; the
 * pixel's primary hit — a triangle and its barycentrics — is carried to where that point of that triangle was one frame ago.
 *
 *   the mark           a scene-owned copy of last frame's render-space triangle positions;
 *   the flow pass      one primary ray through every pixel centre; per pixel the displacement of the hit point and the change of the
 *                      facet normal between the marked and the current positions, plus the instance id of mi355pt_motion.h's ID pass;
 *   the flow-aware     twins of mi355pt_temporal_accumulate[_device] and mi355pt_temporal_accumulate_rectified[_device] that add the
 *   accumulation       pixel's record instead of delta.
 *
 * The per-instance table of mi355pt_motion.h stays: it is cheaper where motion is rigid (no second triangle array, no flow pass).
 * The text below is normative: tests/flow_reference.py restates it in NumPy.
 *
 * THE MARK.  mi355pt_scene_flow_mark copies the render-space leaf-order triangle array (n_tris records of 48 bytes, what
 * mi355pt_scene_export_bvh gives) into an array the scene owns, allocated by the first mark after a build and freed with the scene.  The
 * copy is asynchronous on the stream: order it before the moves of the frame, which are synchronous.  A frame loop marks, then moves,
 * then renders: the mark then holds the positions in the PREVIOUS frame's render space — the previous camera position included, because
 * render space is world space minus the camera position and a camera move rewrites every position.  The three in-place moves keep the
 * mark.  Every mi355pt_scene_build DROPS it, and so does a move that fell back to a build (result.rebuilt = 1): the leaf order is then
 * another one.  After that the caller restarts the accumulation (prev == NULL) and marks again.
 *
 * THE FLOW PASS.  Per pixel p of the launch's shard (8 x 8 tiles dealt out like the ID pass; a pixel outside the shard is not written):
 * the ray camera.sample_ray(p, uv = (0.5, 0.5)), the closest hit as the traversal returns it: the leaf-order triangle index tri and the
 * barycentrics b0, b1, b2 (of the reference's own local-space test where the scene is not in local-triangle mode).  With P0, P1, P2 the
 * three positions of record tri of the CURRENT array and Q0, Q1, Q2 those of the MARKED array:
 *     id   = (instance of the triangle) + 1                     — pixel for pixel what mi355pt_render_ids_device writes;
 *     Xc_i = (b0 P0_i + b1 P1_i) + b2 P2_i,   Xv_i = (b0 Q0_i + b1 Q1_i) + b2 Q2_i,   d_i = Xv_i - Xc_i,   i = 0, 1, 2;
 *     ng(P) = c / sqrtf((c.x c.x + c.y c.y) + c.z c.z),  c = cross(P1 - P0, P2 - P0),  c.x = e1.y e2.z - e1.z e2.y  (and cyclic);
 *     dn   = ng(Q) - ng(P),  or (0, 0, 0) when either squared length is 0 or not finite.
 * A miss writes id = 0, d = dn = 0, pad = 0: all eight words zero.  Every operation is a separate binary32 operation, no fused
 * multiply-add; sqrtf and the divisions are correctly rounded.  A triangle whose two records are bytewise equal therefore gives
 * d = dn = +0 exactly (x - x is +0 for every finite x).  The result does not depend on params->spp, seed or sampler.
 *
 * THE FLOW-AWARE ACCUMULATION is the text of mi355pt_temporal.h (and mi355pt_temporal_rectify.h, which builds on its gather) with
 * exactly these changes, for a pixel p:
 *     Xp = X + flow[p].d  (component by component)  replaces  Xp = X + delta;  view->delta is NOT read: the camera's share is inside d.
 *     nrm' = nrm + flow[p].dn  (component by component)  replaces nrm in the plane test and in the normal test of the taps.
 *     With ids_prev given, a tap q is additionally VALID only if ids_prev[q] == ids_cur[p].
 * Every operation is a separate binary32 operation; the loads of all taps — the id taps included — are unconditional, at indices clamped
 * to the frame; no atomics.  With all-zero records and without ids_prev the outputs are bit-equal to those of the existing call at
 * delta = 0.
 *
 * THE LIMIT OF dn.  A pixel's guide normal is the AVERAGED SHADING normal of its samples; dn is the change of the FACET (geometric)
 * normal at the pixel centre.  Adding it is exact for a translation (dn = 0) and for a flat-shaded surface.  For a rotation R of the
 * triangle it is first order: (R - 1) ng is added where (R - 1) nrm was due, an error of (R - 1)(nrm - ng), the size of the rotation
 * times the distance between shading and geometric normal.  nrm' is NOT renormalised (neither is nrm in mi355pt_temporal.h, nor the
 * table form's under a scale).  Motion seen through a mirror or a glass pane is not followed: the record is the primary hit's.
 */
#ifndef MI355PT_FLOW_H
#define MI355PT_FLOW_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355pt_flow_pixel {   /* 32 bytes, 16-byte aligned records on the device */
    float d[3];      /* X_prev_render - X_cur_render of the pixel's primary hit */
    uint32_t id;     /* instance + 1, or 0 for a miss */
    float dn[3];     /* facet normal before - facet normal now */
    uint32_t pad;    /* 0 */
} mi355pt_flow_pixel;

/* Copies the current render-space triangle positions of a built scene into the scene's mark, asynchronously on `hip_stream`.
 * MI355PT_E_INVALID for a null scene or a scene built with mi355pt_scene_build_multi, MI355PT_E_NOT_BUILT for an unbuilt scene,
 * MI355PT_E_DEVICE when the current HIP device is not the one the scene was built on (or on a HIP error). */
int mi355pt_scene_flow_mark(mi355pt_scene* s, void* hip_stream);
/* 1 while the scene holds a mark that belongs to its current tree, else 0 (also for a null or unbuilt scene). */
int mi355pt_scene_flow_marked(const mi355pt_scene* s);

/* The flow pass on device buffers: ONE launch, asynchronous on `hip_stream`, with the shard rule, the statistics and every refusal of
 * mi355pt_render_ids_device (d_flow in the place of d_ids).  d_ids (W x H u32, NULL ok) receives the ids as well.  Also refused with
 * MI355PT_E_INVALID: a scene without a mark, a d_flow that is not 16-byte aligned, d_flow == d_ids. */
int mi355pt_render_flow_device(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* params, mi355pt_flow_pixel* d_flow /* W*H */,
                               uint32_t* d_ids /* W*H or NULL */, void* hip_stream, mi355pt_stats* stats);
/* The same into host buffers: zeroed device buffers, the launch on the default stream, the copies back (a pixel outside the shard reads
 * 0); flow needs no alignment here. */
int mi355pt_render_flow(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* params, mi355pt_flow_pixel* flow /* W*H */,
                        uint32_t* ids /* W*H or NULL */, mi355pt_stats* stats);

/* The flow-aware accumulation on device buffers: the arguments, the launches and every refusal of mi355pt_temporal_accumulate_device,
 * plus d_flow (W x H records of the current frame, 16-byte aligned), d_ids_cur (W x H u32 of the current frame; may be NULL when
 * d_ids_prev is NULL) and d_ids_prev (of the previous frame; NULL: no id test of the taps).  Without a previous frame (prev == NULL,
 * view == NULL) this IS the existing call: the records and the ids are checked and not read.  Also refused with MI355PT_E_INVALID, before
 * anything touches the device: a NULL d_flow, a d_flow that is not 16-byte aligned, d_ids_prev without d_ids_cur, the records or an id
 * pointer equal to an output pointer. */
int mi355pt_temporal_accumulate_flow_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                            const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                            const mi355pt_temporal_params* params, const uint32_t* d_ids_cur, const uint32_t* d_ids_prev,
                                            const mi355pt_flow_pixel* d_flow, float* d_out_film, float* d_out_half, float* d_out_length,
                                            void* hip_stream);
/* The same with host buffers (ids, records and films), as mi355pt_temporal_accumulate; the records need no alignment here. */
int mi355pt_temporal_accumulate_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                     const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                     const uint32_t* ids_cur, const uint32_t* ids_prev, const mi355pt_flow_pixel* flow, float* out_film,
                                     float* out_half, float* out_length);
/* The rectified form: the arguments and refusals of mi355pt_temporal_accumulate_rectified_device plus the three above; the scratch must
 * not be the records or an id buffer either. */
int mi355pt_temporal_accumulate_rectified_flow_device(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                                      const mi355pt_temporal_view* view, uint32_t width, uint32_t height,
                                                      const mi355pt_temporal_params* params, const mi355pt_temporal_rectify_params* rectify_params,
                                                      void* d_scratch, size_t scratch_bytes, const uint32_t* d_ids_cur, const uint32_t* d_ids_prev,
                                                      const mi355pt_flow_pixel* d_flow, float* d_out_film, float* d_out_half, float* d_out_length,
                                                      void* hip_stream);
int mi355pt_temporal_accumulate_rectified_flow(const mi355pt_temporal_frame* cur, uint32_t spp, const mi355pt_temporal_frame* prev,
                                               const mi355pt_temporal_view* view, uint32_t width, uint32_t height, const mi355pt_temporal_params* params,
                                               const mi355pt_temporal_rectify_params* rectify_params, const uint32_t* ids_cur, const uint32_t* ids_prev,
                                               const mi355pt_flow_pixel* flow, float* out_film, float* out_half, float* out_length);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_FLOW_H */
