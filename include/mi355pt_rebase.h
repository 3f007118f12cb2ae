/*
 * mi355pt_rebase.h — the camera-move block of the C ABI (included by mi355pt.h right after mi355pt_robust.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference builds its scene once per frame (scene.rs:64-76).  mi355pt_scene_build bakes the camera
 * position into the device records (render space = world - position).  A camera TRANSLATION changes the render-space vertex positions, the
 * boxes of the two trees (exact min / max of those vertices, plus the pad of the 4-wide tree), the instance matrices' translation and
 * numeric inverse, the delta lights' positions, the emissive triangles' records and four scalars — and nothing else: not the topology of the
 * tree, not the shading records, textures, tables or environment maps.  mi355pt_scene_move_camera recomputes exactly that, in place:
 *
 *   host     the instance records, the light list, the emissive triangles, tri_shift / shared_mw — with the lowering's own functions —
 *            and uploads them into the existing allocations;
 *   device   1. one thread per leaf-order triangle: the 9 render-space position floats from the local record and the instance matrix, in
 *               the lowering's operation order ((m0 x + m4 y) + m8 z) + m12, and the count of triangles that became degenerate;
 *            2. the BVH2's boxes bottom-up, one launch per node height (the kernel boundary orders the levels; no flags between
 *               workgroups): a leaf's box from its triangles, a node's as the union of its two child boxes;
 *            3. one thread per child slot of the 4-wide tree: the box of the BVH2 (node, side) it carries, padded as the lowering pads.
 *
 * Host and device are compiled without floating-point contraction, min / max pick the same zero when -0.0 meets +0.0
 * (csrc/rebase_plan.hpp), and so the result is held to bytes: after MI355PT_OK every device array equals what the host lowering produces
 * for the new camera with the topology pinned to the built tree (mi355pt_scene_debug_move_digest against mi355pt_scene_debug_device_digest,
 * include/mi355pt_debug.h).  The tree keeps the topology it was built with: its SAH quality is that of the build position.
 */
#ifndef MI355PT_REBASE_H
#define MI355PT_REBASE_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi355pt_move_result.reason */
enum {
    MI355PT_MOVE_REBASED = 0,                  /* re-based in place */
    MI355PT_MOVE_SAME_POSITION = 1,            /* the position is the built one: nothing done */
    MI355PT_MOVE_DEGENERATE_SET_CHANGED = 2,   /* rebuilt: a triangle of the tree has an exactly zero cross product at the new position, or one left out no longer has */
    MI355PT_MOVE_INSTANCE_CLASS_CHANGED = 3,   /* rebuilt: an instance's pure-translation flag, or the scene's local-triangle mode, would come out differently */
    MI355PT_MOVE_UNSUPPORTED_BUILD = 4         /* rebuilt: the library was compiled with quantised 4-wide nodes (PT_NODE_Q16) */
};

typedef struct mi355pt_move_result {
    uint32_t rebuilt;      /* 0: re-based in place; 1: the call fell back to a full mi355pt_scene_build */
    uint32_t reason;       /* MI355PT_MOVE_* */
    uint32_t launches;     /* kernel launches issued (0 when rebuilt or same position): 2 + the number of node heights of the BVH2 */
    double host_ms;        /* wall time of the call */
    double device_ms;      /* HIP-event time from the first launch to the last (0 without launches) */
} mi355pt_move_result;

/* Moves the camera of a built scene to cam->position.  After MI355PT_OK the scene is in the state mi355pt_scene_build(s, cam) would leave
 * it in, except that the tree keeps the topology it was built with; every later render call must pass the new position.  Synchronous: waits
 * for its own launches; the caller has no render in flight on the scene (one thread, one stream per scene, as everywhere).
 * Falls back to mi355pt_scene_build (rebuilt = 1, reason says why) whenever re-basing would not give what a fresh lowering gives.
 * Errors: MI355PT_E_INVALID for a null scene or camera and for a scene built with mi355pt_scene_build_multi (not supported);
 * MI355PT_E_NOT_BUILT for an unbuilt scene; MI355PT_E_DEVICE when the current HIP device is not the one the scene was built on, or on a HIP
 * error — after which the scene must be built again. */
int mi355pt_scene_move_camera(mi355pt_scene* s, const mi355pt_camera* cam, mi355pt_move_result* out /* NULL ok */);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_REBASE_H */
