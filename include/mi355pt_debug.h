/* mi355pt_debug.h — test and diagnosis surface of libmi355pt.so.
 *
 * Everything here is used by the parity tests (tests/), the tools under tools/ and bench.py's instrumented launch; nothing here is needed
 * to drop the library in behind renderer::render() (that is include/mi355pt.h).  The probes run the SAME device functions as the render
 * path, and the per-sample log is written by the production kernel itself, which is why they live in the product library
 * rather than in a test build of it. */
#ifndef MI355PT_DEBUG_H
#define MI355PT_DEBUG_H
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mi355pt_params.rr_gate_slack (and nothing else) changes what a render call computes for diagnostic purposes; it is honoured only after
 * mi355pt_debug_unlock(1) and refused otherwise.  Process-wide; mi355pt_debug_unlock(0) locks again.  Returns the previous state. */
int mi355pt_debug_unlock(int on);

/* How the next mi355pt_scene_build lowers the instances (A/B runs and tests; the three paths must give the reference's hit alike):
 * 0 (default) the triangle array holds LOCAL vertices when every instance is the same pure translation - every triangle test of every
 *   traversal is then the reference's (primitive/impls/triangle_mesh.rs:89-119) - else render-space triangles and the triangle found is
 *   intersected again in its mesh's local space; 1 never the local array; 2 in addition every instance through the full matrix path. */
int mi355pt_scene_debug_set_lowering(mi355pt_scene* s, int mode);

/* What mi355pt_scene_build would lower this scene to for `cam`, without a device: the lowering's two stages around the HOST tree builder
 * (whatever mi355pt_scene_set_bvh_builder says), nothing uploaded, the scene - built or not - left as it is.  digests[i] is the FNV-1a-64
 * of the raw bytes of one array, in upload order, and the last one that of the scalars (the non-pointer fields of the device's scene record
 * in declaration order, the feature bits, the degenerate count, the BVH2 depth, the 4-wide node count, the stack need, the collapse
 * method); pointers inside hashed records count as null.  names_buf receives one name per digest, each followed by a newline, then the
 * text mi355pt_scene_info would give without its three *_ms fields.  *n: capacity of digests on entry, their number on return (also when
 * a buffer is too small, which is refused).  tests/golden/scene_lowering_digests.json holds the values of the test scenes. */
int mi355pt_scene_debug_lowering_digest(const mi355pt_scene* s, const mi355pt_camera* cam, char* names_buf, size_t names_len,
                                        uint64_t* digests, uint32_t* n);

/* The camera-ray candidate lists of the production kernels (csrc/camera_candidates.hpp), computed on the host: lowers the scene for `cam`
 * like mi355pt_scene_debug_lowering_digest (no device, the scene left as it is) and runs the header's walk over the lowered 4-wide tree
 * for each of n_rects pixel rectangles (rects: x0, y0, x1, y1 per rectangle, inclusive; the kernels' rectangle is a work item's pixel
 * block).  Rectangle r: out_counts[r] leaf-order triangle indices in out_indices[r * cap ...] (NULL ok), out_overflow[r] != 0 when more than
 * `cap` triangles qualify and the list is incomplete (cap 1 .. 4096; the kernels' is 16).  out_tris (NULL ok): the lowered triangles in leaf
 * order, 9 floats each, RENDER space; *n_tris (NULL ok) holds its capacity in triangles on entry and the triangle count on return.
 * Nothing on the render path calls this: tests/test_camera_candidates*.py and tools/camera_list_stats.py do. */
int mi355pt_scene_debug_camera_candidates(const mi355pt_scene* s, const mi355pt_camera* cam, const uint32_t* rects, uint32_t n_rects, uint32_t cap,
                                          uint32_t* out_counts, uint8_t* out_overflow, uint32_t* out_indices, float* out_tris, uint32_t* n_tris);

/* mi355pt_scene_move_camera (include/mi355pt_rebase.h) on the host: the digests, in mi355pt_scene_debug_lowering_digest's format and order, of
 * the scene lowered for `cam_new` with the topology PINNED to the tree of `cam_built` — stage A for cam_new; the BVH2 of cam_built (its links
 * and leaf order) with every box recomputed from the new triangles; stage B; then cam_built's 4-wide collapse with its boxes copied from that
 * BVH2 and padded.  The tree of cam_built is the host builder's, except that a scene whose tree WAS built at cam_built's position by the GPU
 * builder — wherever mi355pt_scene_move_camera has taken it since — pins to that tree (the build keeps it on the host).  No device, the scene left as it is.  *out_reason (NULL ok): the MI355PT_MOVE_* reason
 * a move from cam_built to cam_new would report; for the two reasons that rebuild, the digests are those of a fresh lowering for cam_new.
 * With cam_new = cam_built the digests are mi355pt_scene_debug_lowering_digest's: the refit and the pad reproduce the builders' boxes. */
int mi355pt_scene_debug_move_digest(const mi355pt_scene* s, const mi355pt_camera* cam_built, const mi355pt_camera* cam_new, char* names_buf,
                                    size_t names_len, uint64_t* digests, uint32_t* n, uint32_t* out_reason);
/* The tree of that pinned lowering in mi355pt_scene_export_bvh's layout and calling convention (NULL buffers for the counts), host only; and
 * out_pad_radii (2 floats, NULL ok): the largest coordinate magnitude the pad of the 4-wide tree is scaled by, {as the move computes it from
 * the BVH2 root record's two child boxes, as the lowering's own loop over the unpadded 4-wide boxes computes it}. */
int mi355pt_scene_debug_move_export(const mi355pt_scene* s, const mi355pt_camera* cam_built, const mi355pt_camera* cam_new, void* out_nodes,
                                    uint32_t* n_nodes, void* out_tris, uint32_t* n_tris, int32_t* root, float* out_pad_radii);
/* The same digests of what the DEVICE holds: reads back every array of a built scene and hashes it the same way, in upload order, with the
 * scalars' digest last; pointers inside hashed records count as null.  The text after the names is mi355pt_scene_info's without its *_ms
 * fields.  Needs the scene's device current. */
int mi355pt_scene_debug_device_digest(const mi355pt_scene* s, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n);

/* mi355pt_scene_move_instances (include/mi355pt_instances.h) on the host: the digests, in mi355pt_scene_debug_lowering_digest's format and
 * order, of the host lowering of the BUILT scene's CURRENT description (the matrices the moves left) for `cam`, over the topology the built
 * scene holds — the build keeps both trees on the host, whichever builder made them — with every box refit from the new triangles by the
 * functions the kernels call.  No device, the scene left as it is.  At unchanged transforms and the built camera the digests are
 * mi355pt_scene_debug_lowering_digest's under the host builder.  MI355PT_E_NOT_BUILT for an unbuilt scene; MI355PT_E_INVALID when the
 * description no longer lowers over that tree (another degenerate set, another instance class): only a rebuild serves it. */
int mi355pt_scene_debug_pinned_digest(const mi355pt_scene* s, const mi355pt_camera* cam, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n);
/* The BVH2 of that pinned lowering in mi355pt_scene_export_bvh's layout and calling convention (NULL buffers for the counts), host only, and
 * (n_entries NULL: not wanted) the refit plan's (node << 1 | side) entries in the order the SAH cost sums their terms. */
int mi355pt_scene_debug_pinned_export(const mi355pt_scene* s, const mi355pt_camera* cam, void* out_nodes, uint32_t* n_nodes, void* out_tris, uint32_t* n_tris,
                                      int32_t* root, uint32_t* out_entries, uint32_t* n_entries);
/* The two calls above without a device: mi355pt_scene_debug_pin_host_tree lowers an UNBUILT scene for `cam` with the host builder and keeps
 * what a build keeps on the host (both trees, the instance classes, the left-out triangles, the light records) — no device array exists and
 * the scene stays unbuilt for every other call; mi355pt_scene_debug_set_instance_transform then replaces a local_to_world matrix (column-major
 * 4x4) of the description of such a scene, as mi355pt_scene_move_instances does on a built one, without any check of the matrix.  Both
 * refuse a built scene with MI355PT_E_INVALID. */
int mi355pt_scene_debug_pin_host_tree(mi355pt_scene* s, const mi355pt_camera* cam);
int mi355pt_scene_debug_set_instance_transform(mi355pt_scene* s, uint32_t instance, const float* local_to_world);
/* ... and mi355pt_scene_debug_set_mesh_vertices replaces vertex arrays of the description of such a scene, as mi355pt_scene_deform_meshes
 * (include/mi355pt_deform.h) does on a built one, with that call's checks of the arrays (ids, a tangent without uv, non-finite positions)
 * and its normalisation of the normals: the description update alone, so that mi355pt_scene_debug_pinned_digest and
 * mi355pt_scene_debug_pinned_export give the host form of a deformation without a device.  Refuses a built scene with MI355PT_E_INVALID. */
int mi355pt_scene_debug_set_mesh_vertices(mi355pt_scene* s, const mi355pt_mesh_update* updates, uint32_t n);
/* ... and mi355pt_scene_debug_apply_edits replaces material, delta-light and environment-light descriptions of such a scene, as
 * mi355pt_scene_edit (include/mi355pt_edit.h) does on a built one, with that call's checks of the edits (ids, the add calls' validators,
 * texture and LUT ids of the pin, non-finite values, singular light matrices): the description update alone, so that
 * mi355pt_scene_debug_pinned_digest gives the host form of an edit without a device.  Refuses a built scene with MI355PT_E_INVALID. */
int mi355pt_scene_debug_apply_edits(mi355pt_scene* s, const mi355pt_scene_edits* edits);
/* The host form of the SAH cost mi355pt_scene_move_instances reports (csrc/instance_move_plan.hpp sah_cost_host): node records as
 * mi355pt_scene_export_bvh gives them, the entries of mi355pt_scene_debug_pinned_export.  No device. */
int mi355pt_debug_sah_cost(const void* nodes, uint32_t n_nodes, int32_t root, const uint32_t* entries, uint32_t n_entries, float* out_cost);

/* ---------------- probes (parity tests; same device code as the render path) ---------------- */
/* The built acceleration structure as the device holds it (no reference counterpart; the reference's is scene/src/bvh.rs:300-343):
 * node records of 64 B {bx[4] = lo0.x lo1.x hi0.x hi1.x, by[4], bz[4], int32 child[2] (>= 0 node index, < 0 leaf:
 * first = (c & 0x7fffffff) >> 3, count = (c & 7) + 1), pad[2]} and leaf-ordered render-space triangle records of 48 B
 * {p0 p1 p2 as 9 floats, pad[3]}.  Call with NULL buffers for the counts; *n_nodes / *n_tris hold the buffer capacities on
 * entry.  The parity tests hand the tree to the oracle, which walks it to check the instrumented kernel's step counts. */
int mi355pt_scene_export_bvh(const mi355pt_scene* s, void* out_nodes, uint32_t* n_nodes, void* out_tris, uint32_t* n_tris,
                             int32_t* root);
/* Host-only check of the acceleration structure the render path walks (no reference counterpart): builds the sweep-SAH BVH2 over the
 * n_tris triangles (9 floats each), collapses it to the 4-wide tree of the cooperative traversals and walks BOTH on the CPU for n_rays rays
 * (6 floats each: origin, direction): out_mismatch = rays for which the two trees reach different sets of leaves (must be 0);
 * out_info[4] = {BVH2 nodes, BVH4 nodes, BVH2 depth, worst-case stack entries of the BVH4 (< 24 by construction)}. */
int mi355pt_probe_bvh_collapse(const float* tri_pos, uint32_t n_tris, const float* rays_od, uint32_t n_rays, uint32_t* out_info,
                               uint32_t* out_mismatch);
/* The same collapse + validation on a caller-supplied BVH2 (n_nodes 64-byte records in the layout mi355pt_scene_export_bvh writes; leaves
 * are links < 0 holding first << 3 | count - 1): the guard SceneImpl::build runs before any tree reaches the device, reachable without a
 * device.  out_info = {nodes2, nodes4, 1 if the cost-optimal collapse ran (0: greedy), worst-case per-lane stack entries}; a tree the
 * 24-entry LDS stack cannot serve (too deep, broken links, triangles lost) is refused with MI355PT_E_INVALID.  Host only. */
int mi355pt_probe_bvh_collapse_nodes(const void* bvh2_nodes, uint32_t n_nodes, int32_t root, uint32_t n_tris, uint32_t* out_info /* 4 */);
/* ZSobolSampler: for each query (x, y, sample_index) emit n_dims raw 32-bit Sobol outputs following the draw
 * pattern string `pattern` of '1' (get_1d) and '2' (get_2d) characters.  z_sobol_sampler.rs:198-230 */
int mi355pt_probe_sobol(uint32_t width, uint32_t height, uint32_t spp, uint32_t seed, const uint32_t* xys /* n*3 */,
                        uint32_t n, const char* pattern, uint32_t* out_bits /* n * n_values(pattern) */);
/* sin / cos as the render kernels compute them (csrc/pt_libm.hpp: the host libm's algorithm restated; the reference calls f32::sin_cos,
 * e.g. scene/src/material/bsdf/dielectric.rs:77-112 via common.rs) for the n floats with bit patterns first_bits + i * stride, compared on
 * the host with sinf / cosf of THIS machine's libm: out_counts[3] = {compared, sin results that differ in any bit, cos results}. */
int mi355pt_probe_sincos(uint32_t first_bits, uint32_t stride, uint32_t n, uint64_t* out_counts /* 3 */);
/* The two launches of mi355pt_display_meter_device (include/mi355pt_display.h) on the default stream with a HIP event between them: out_ms[2] =
 * {the block histograms, the one-block finish} in milliseconds.  No previous record, no histogram output; the same argument checks;
 * synchronises.  For tools/display_rate.py: the public entry point gives no place to put an event. */
int mi355pt_probe_display_meter_ms(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* params, void* d_scratch,
                                   size_t scratch_bytes, uint32_t* d_record, float* out_ms /* 2 */);
/* Scene::intersect for n rays (render space).  out_t < 0 means miss.  scene.rs:80-90 */
int mi355pt_probe_intersect(const mi355pt_scene* s, const float* origins, const float* dirs, uint32_t n, float* out_t,
                            uint32_t* out_instance, uint32_t* out_triangle, float* out_normal /* n*3 geometric, NULL ok */);
/* Scene::intersect_p for n rays.  scene.rs:93-103 */
int mi355pt_probe_occluded(const mi355pt_scene* s, const float* origins, const float* dirs, const float* t_max, uint32_t n,
                           uint8_t* out_hit);
/* BaseSrgbRenderer::render's per-sample result before the sensor (base_renderer.rs:160-276: the L handed to
 * Sensor::add_sample with its SampledWavelengths): L[4], lambda[4], pdf[4] for every finished path of a render call,
 * written by the PRODUCTION kernel in the launch shape mi355pt_render_accum_device takes for the same arguments
 * (a wave-uniform branch at path end; nothing else differs).  Record r = (k * 64 + (y & 7) * 8 + (x & 7)) *
 * (sample_end - sample_begin) + (sample - sample_begin), k = position of the pixel's 8x8 tile among the tiles of the
 * shard (tile t = shard_index + k * shard_count, row-major tiles); records of pixels outside the frame stay zero.
 * Needs a power-of-two spp.  out_accum (host, W*H*3, NULL ok) receives the linear film sums of the same launch. */
int mi355pt_sample_log_records(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t sample_begin, uint32_t sample_end,
                               size_t* out_records);
int mi355pt_render_sample_log(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t sample_begin,
                              uint32_t sample_end, float* out_L, float* out_lambda, float* out_pdf, size_t n_records,
                              float* out_accum);
/* The same records picked for n (x, y, sample) queries of the whole-frame, whole-job launch (small frames only). */
int mi355pt_probe_radiance(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const uint32_t* xys,
                           uint32_t n, float* out_L, float* out_lambda, float* out_pdf);

/* ---------------- per-pixel motion (include/mi355pt_flow.h) ---------------- */
/* mi355pt_render_flow with the hit it was computed from: the same kernel compiled with one more flag, which also writes per pixel
 * {u32 tri, f32 b0, b1, b2} — the leaf-order triangle and the barycentrics as the traversal returned them; a miss writes four zero words,
 * a pixel outside the shard reads 0 — into out_hits (host, W x H x 16 bytes).  Host buffers; the checks of mi355pt_render_flow. */
int mi355pt_render_flow_debug(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* params, mi355pt_flow_pixel* flow /* W*H */,
                              uint32_t* ids /* W*H or NULL */, void* out_hits /* W*H*16 bytes */, mi355pt_stats* stats);
/* The mark's triangle array (mi355pt_scene_flow_mark) in mi355pt_scene_export_bvh's triangle layout and calling convention: out_tris NULL
 * for the count; *n_tris holds the buffer's capacity on entry.  Synchronises the device.  MI355PT_E_INVALID for a scene without a mark. */
int mi355pt_scene_export_flow_mark(const mi355pt_scene* s, void* out_tris, uint32_t* n_tris);
/* Which triangle of which instance a leaf-order triangle is, as the device's shading records say: out_ids[2 i] = the instance (the index
 * mi355pt_scene_add_instance returned), out_ids[2 i + 1] = the triangle's index inside its mesh.  Same calling convention (out_ids NULL for
 * the count).  The tests compare the flow pass's hits with the oracle's (primitive, triangle) through it. */
int mi355pt_scene_export_triangle_ids(const mi355pt_scene* s, uint32_t* out_ids /* 2 per triangle */, uint32_t* n_tris);


#ifdef __cplusplus
}
#endif
#endif
