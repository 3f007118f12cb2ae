/*
 * mi355pt_deform.h — the mesh-deformation block of the C ABI (included by mi355pt.h right after mi355pt_motion.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference builds its scene once per frame (scene.rs:64-76).  mi355pt_scene_move_camera
 * (mi355pt_rebase.h) moves the camera of a built scene and mi355pt_scene_move_instances (mi355pt_instances.h) its rigid objects;
 * mi355pt_scene_deform_meshes replaces the VERTICES of some meshes — a skinned character, cloth, a morph target, a wave on a surface — and
 * brings the device records up to date in place.  The vertex and triangle counts and the index buffer of a mesh stay what
 * mi355pt_scene_add_mesh took.
 *
 *   host     the description (positions; normals through the normalisation mi355pt_scene_add_mesh applies; tangents), the local boxes of
 *            the updated meshes, the light list and the emissive triangles — with the lowering's own functions —, and for every emissive
 *            instance of an updated mesh its WORLD-space area tables: DevLight::area_sum, every light triangle's cdf, and light_pdf_area per
 *            triangle; uploaded into the existing allocations.  The new arrays of all updated meshes go to the device in ONE staging buffer,
 *            beside a per-instance table (the instance's slot in that buffer, or none) and, once per build and mesh, the mesh's index buffer;
 *   device   1. the LOCAL records of the leaf-order triangles of the updated meshes (deform_tris_kernel): the three positions and rows 0 - 2
 *               of the shading record (vertex normals, tangent), gathered from the staging buffer through the index buffer.  The kernel only
 *               moves bytes; a triangle of another mesh is not written;
 *            2. the render-space positions of ALL leaf-order triangles and the count of triangles that became degenerate (the camera move's
 *               kernel);
 *            3. the shading records of the instances of the updated meshes: the geometric normal ng from the new local vertices, and
 *               light_pdf_area of emissive triangles (the instance move's shade_refresh_kernel);
 *            4. the BVH2's boxes bottom-up, one launch per node height, and the slots of the 4-wide tree (the camera move's kernels);
 *            5. the SAH cost of the refit BVH2 in two launches (the instance move's kernels, its fixed order).
 *
 * launches = 6 + the number of node heights of the BVH2: local records, positions, shading records, one per height, the 4-wide tree, two
 * for the cost.  (A scene whose root is a leaf has no heights, no 4-wide refit and no cost launches: 3.)  The first move after a build runs
 * the two cost launches once more, ahead of everything, for sah_built; they are not counted.
 *
 * As for the two other moves the result is held to bytes: after MI355PT_OK every device array equals what the host lowering produces for
 * the updated description with the topology pinned to the built tree (mi355pt_scene_debug_pinned_digest against
 * mi355pt_scene_debug_device_digest, include/mi355pt_debug.h), and sah_built / sah_after are bit-equal to the host's sum in the same order.
 *
 * A deformation changes no matrix, so neither class of the lowering can change: no mark is needed before the build, and the call works in
 * local-triangle mode (the triangle array the traversals read IS the local one there, and the render-space array is re-derived from it).
 *
 * LIMITS.  Refit only: the tree keeps the topology it was built with, and a mesh bent far from its built shape leaves boxes that overlap —
 * sah_after / sah_built says by how much, rebuild_above turns it into a rebuild.  A triangle that becomes or stops being degenerate (an
 * exactly zero cross product, in the space the lowering decides it in) rebuilds.  No topology change, no device-pointer input: the
 * description on the host holds the vertices for the fallback and the digests.  Scenes built with mi355pt_scene_build_multi are not
 * deformed.  The temporal accumulation (mi355pt_temporal.h) assumes a static world and the object motion vectors of mi355pt_motion.h a
 * rigid motion per instance: neither reprojects across a deformation — start those accumulations again after this call, or use the
 * per-pixel motion records of mi355pt_flow.h, which follow it.
 */
#ifndef MI355PT_DEFORM_H
#define MI355PT_DEFORM_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi355pt_instance_move_result.reason of mi355pt_scene_deform_meshes: MI355PT_MOVE_REBASED (deformed in place),
 * MI355PT_MOVE_DEGENERATE_SET_CHANGED and MI355PT_MOVE_UNSUPPORTED_BUILD of mi355pt_rebase.h, MI355PT_MOVE_SAH_DEGRADED of
 * mi355pt_instances.h, and: */
enum { MI355PT_MOVE_SAME_VERTICES = 7 };   /* every given array is bytewise the current one: nothing done, 0 launches */

typedef struct mi355pt_mesh_update {
    uint32_t geom;             /* id from mi355pt_scene_add_mesh */
    const float* pos;          /* n_vert x 3, required */
    const float* nrm;          /* n_vert x 3, or NULL = keep the current normals */
    const float* tri_tangent;  /* n_tri x 3, or NULL = keep; refused (not NULL) for a mesh without uv */
} mi355pt_mesh_update;

/* Replaces the vertex arrays of n meshes (geom ids strictly ascending) of a built scene and brings the device records of EVERY instance of
 * those meshes up to date in place.  `cam` is the camera the scene is at (its position must be the built / last moved one).  Synchronous,
 * like mi355pt_scene_move_instances, whose params and result it shares: rebuild_above, sah_built, sah_after, launches, host_ms and
 * device_ms mean what they mean there.  Falls back to mi355pt_scene_build of the updated description (rebuilt = 1, reason says why); after
 * MI355PT_OK the host description holds the new arrays in every case.  Normals are normalised twice, like mi355pt_scene_add_mesh's; "the
 * current one" of MI355PT_MOVE_SAME_VERTICES compares the normalised normals.
 * Refused before anything touches the device or the description: MI355PT_E_INVALID for null arguments, n = 0, a geom id out of range or
 * ids not strictly ascending, a null pos, a tangent for a mesh without uv, a non-finite position, a camera position other than the scene's,
 * a scene built with mi355pt_scene_build_multi; MI355PT_E_NOT_BUILT for an unbuilt scene; MI355PT_E_DEVICE when the current HIP device is
 * not the one the scene was built on.  MI355PT_E_DEVICE on a HIP error — after which the scene must be built again. */
int mi355pt_scene_deform_meshes(mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_mesh_update* updates, uint32_t n,
                                const mi355pt_instance_move_params* p /* NULL = defaults */, mi355pt_instance_move_result* out /* NULL ok */);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_DEFORM_H */
