/*
 * mi355pt_instances.h — the instance-move block of the C ABI (included by mi355pt.h right after mi355pt_rebase.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference builds its scene once per frame (scene.rs:64-76).  mi355pt_scene_move_camera
 * (mi355pt_rebase.h) moves the camera of a built scene; mi355pt_scene_move_instances moves OBJECTS of it: it replaces the local_to_world
 * matrices of some instances and brings the device records up to date in place.  A general transform changes more than a camera
 * translation does:
 *
 *   host     the instance records, the light list and the emissive triangles — with the lowering's own functions —, and for every moved
 *            emissive instance its WORLD-space area tables: DevLight::area_sum, every light triangle's cdf, and light_pdf_area per
 *            triangle; uploaded into the existing allocations;
 *   device   1. the render-space positions of ALL leaf-order triangles (the camera move's kernel: a pure function of the local record and
 *               the matrix, so an unmoved triangle gets its own bytes again) and the count of triangles that became degenerate;
 *            2. the shading records of the moved instances: the geometric normal ng through the new inverse-transpose, in the lowering's
 *               operation order, and light_pdf_area of emissive triangles (shade_refresh_kernel);
 *            3. the BVH2's boxes bottom-up, one launch per node height, and the slots of the 4-wide tree (the camera move's kernels);
 *            4. the SAH cost of the refit BVH2, a fixed-order sum in two launches: sum over every child box of
 *               half_area x (1 for an inner child, the triangle count for a leaf), divided by the half area of the root;
 *               half_area = (dx dy + dy dz) + dz dx in binary32.
 *
 * launches = 5 + the number of node heights of the BVH2: positions, shading records, one per height, the 4-wide tree, two for the cost.
 * (A scene whose root is a leaf has no heights, no 4-wide refit and no cost launches: 2.)  The first move after a build runs the two cost
 * launches once more, ahead of everything, for sah_built; they are not counted.
 *
 * As for the camera move the result is held to bytes: after MI355PT_OK every device array equals what the host lowering produces for the
 * updated description with the topology pinned to the built tree (mi355pt_scene_debug_pinned_digest against
 * mi355pt_scene_debug_device_digest, include/mi355pt_debug.h), and sah_built / sah_after are bit-equal to the host's sum in the same order.
 *
 * LIMITS.  Refit only: the tree keeps the topology it was built with, and an object carried across the room leaves boxes that overlap —
 * sah_after / sah_built says by how much, rebuild_above turns it into a rebuild.  The two classes of the lowering cannot change in place: an
 * instance that was lowered as a pure translation stays one (give it a rotation and the call rebuilds), and a scene in local-triangle mode
 * rebuilds on every move — mark what will move with mi355pt_scene_set_instance_dynamic BEFORE the build.  A triangle that becomes or
 * stops being degenerate (an exactly zero cross product in render space) rebuilds.  Scenes built with mi355pt_scene_build_multi are not
 * moved.  The temporal accumulation (mi355pt_temporal.h) reprojects a hit into the previous CAMERA and assumes a static world: across an
 * instance move accumulate with the object motion vectors of mi355pt_motion.h (the ID pass, the motion table, the motion-aware twins).
 */
#ifndef MI355PT_INSTANCES_H
#define MI355PT_INSTANCES_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi355pt_instance_move_result.reason: MI355PT_MOVE_REBASED (moved in place), MI355PT_MOVE_DEGENERATE_SET_CHANGED,
 * MI355PT_MOVE_INSTANCE_CLASS_CHANGED and MI355PT_MOVE_UNSUPPORTED_BUILD of mi355pt_rebase.h, and: */
enum {
    MI355PT_MOVE_SAME_TRANSFORMS = 5,          /* every given matrix is bytewise the current one: nothing done, 0 launches */
    MI355PT_MOVE_SAH_DEGRADED = 6              /* rebuilt: sah_after / sah_built exceeded rebuild_above */
};

/* before mi355pt_scene_build: this instance will be moved.  It is lowered through the general matrix path whatever its transform is
 * (DevInstance::identity = 0) and the scene does not use the local-triangle mode (DevScene::tris_are_local = 0), so that no later
 * transform changes a class.  Default off: a scene that never calls this lowers to the bytes it lowers to today.
 * Errors: MI355PT_E_INVALID for a null scene, an instance out of range, or a built scene (the mark takes effect at a build). */
int mi355pt_scene_set_instance_dynamic(mi355pt_scene* s, uint32_t instance, uint32_t dynamic);

typedef struct mi355pt_instance_move_params {
    float rebuild_above;   /* 0 = never; else: build again when sah_after / sah_built exceeds it */
} mi355pt_instance_move_params;

typedef struct mi355pt_instance_move_result {
    uint32_t rebuilt, reason, launches;      /* reason: MI355PT_MOVE_* of mi355pt_rebase.h plus the new ones above */
    float sah_built, sah_after;              /* SAH cost of the BVH2 at the last build / after this refit (0 when rebuilt) */
    double host_ms, device_ms;
} mi355pt_instance_move_result;

/* Sets the local_to_world matrices (column-major 4x4) of n instances (ids strictly ascending) of a built scene and brings the device
 * records up to date in place.  `cam` is the camera the scene is at (its position must be the built / last moved one).  Synchronous, like
 * mi355pt_scene_move_camera.  Falls back to mi355pt_scene_build of the updated description (rebuilt = 1, reason says why); after MI355PT_OK
 * the host description holds the new matrices in every case.  sah_built: the cost of the tree as the first move after the last build found
 * it; both costs are 0 when the call rebuilt, did nothing, or the root is a leaf.
 * Refused before anything touches the device, the scene left as it was: MI355PT_E_INVALID for null arguments, n = 0, an id out of range
 * or ids not strictly ascending, a non-finite or singular matrix (the lowering's own test), a camera position other than the scene's, a
 * scene built with mi355pt_scene_build_multi; MI355PT_E_NOT_BUILT for an unbuilt scene; MI355PT_E_DEVICE when the current HIP device is
 * not the one the scene was built on.  MI355PT_E_DEVICE on a HIP error — after which the scene must be built again. */
int mi355pt_scene_move_instances(mi355pt_scene* s, const mi355pt_camera* cam, const uint32_t* ids, const float* local_to_world /* n x 16 */,
                                 uint32_t n, const mi355pt_instance_move_params* p /* NULL = defaults */, mi355pt_instance_move_result* out /* NULL ok */);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_INSTANCES_H */
