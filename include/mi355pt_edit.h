/*
 * mi355pt_edit.h — the lights-and-materials block of the C ABI (included by mi355pt.h right after mi355pt_budget.h: a caller of mi355pt.h has it).
 *
 * EXTENSION, no reference counterpart: the reference builds its scene once per frame (scene.rs:64-76).  mi355pt_scene_move_camera
 * (mi355pt_rebase.h), mi355pt_scene_move_instances (mi355pt_instances.h) and mi355pt_scene_deform_meshes (mi355pt_deform.h) change where
 * things are; mi355pt_scene_edit changes what they LOOK like and how they are lit — a material's parameters or its type, a point / spot /
 * directional light's position, kind, intensity and spectrum, an environment light's intensity, rotation and map — and brings the device
 * records up to date in place.  No triangle and no box changes, so the tree, the flow mark of mi355pt_flow.h and the camera candidate
 * lists stay what they are.
 *
 *   host     the description takes the edited records; then, with the lowering's own functions: the material records (the hidden
 *            materials of the delta and environment lights included) with their texture descriptors, the coat-albedo row of a clearcoat
 *            material that changed, the delta lights' records (a directional light's area from the mesh bounds the build keeps), the record,
 *            the tables and the integrated spectrum of an edited environment light, and the feature bits the kernel selector reads.  What
 *            differs bytewise from the built records is uploaded into the existing allocations: the material array, the coat-albedo table,
 *            the light array, the environment records, the three tables of an environment whose map changed;
 *   device   ONE kernel, and only when a material's queue sort class (its type, + 8 with a spectrum texture) changed: the class word of the
 *            leaf-order triangles of that material in the local and the render-space triangle records (reclass_tris_kernel).  The kernel
 *            only moves bytes; a triangle of another material is not written.
 *
 * launches = 0 or 1.  The scene's feature set follows the edited materials: the next render selects its kernel from them
 * (features_before / features_after say whether another kernel will run).
 *
 * As for the other updates the result is held to bytes: after MI355PT_OK every device array equals what the host lowering produces for the
 * edited description with the topology pinned to the built tree (mi355pt_scene_debug_pinned_digest against
 * mi355pt_scene_debug_device_digest, include/mi355pt_debug.h).
 *
 * LIMITS.  A material that becomes or stops being MI355PT_MAT_EMISSIVE changes the light list, the light triangles and every shading
 * record's light index: the call builds again.  So does a change of the NUMBER of clearcoat materials (the coat-albedo table is sized by
 * it; MI355PT_MAT_SIMPLE_PBR counts as one).  Textures and LUTs are those of the build: an id added after it is refused.  An environment
 * map keeps the size it was added with.  Scenes built with mi355pt_scene_build_multi are not edited.  The plain temporal accumulation
 * (mi355pt_temporal.h) averages a change of illumination over its history; the rectified one (mi355pt_temporal_rectify.h) follows it.
 */
#ifndef MI355PT_EDIT_H
#define MI355PT_EDIT_H

#include "mi355pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mi355pt_edit_result.reason: MI355PT_MOVE_REBASED (edited in place) and MI355PT_MOVE_UNSUPPORTED_BUILD of mi355pt_rebase.h, and: */
enum {
    MI355PT_EDIT_SAME_RECORDS = 8,        /* every lowered record is bytewise what it was: nothing uploaded, 0 launches */
    MI355PT_EDIT_EMITTER_SET_CHANGED = 9, /* a material became or stopped being MI355PT_MAT_EMISSIVE: built again */
    MI355PT_EDIT_TABLE_SHAPE_CHANGED = 10 /* the number of clearcoat materials changed: built again */
};

typedef struct mi355pt_material_edit {
    uint32_t mat; /* id from mi355pt_scene_add_material */
    mi355pt_material_desc desc;
} mi355pt_material_edit;
typedef struct mi355pt_light_edit {
    uint32_t light; /* index in the order of mi355pt_scene_add_delta_light calls */
    mi355pt_light_desc desc;
} mi355pt_light_edit;
typedef struct mi355pt_env_edit {
    uint32_t env; /* index in the order of mi355pt_scene_add_environment_light calls */
    float intensity;
    const float* local_to_world; /* 16 floats, NULL = keep */
    const float* rgb;            /* width x height x 3 of the size it was added with, NULL = keep the map */
} mi355pt_env_edit;
typedef struct mi355pt_scene_edits {
    const mi355pt_material_edit* materials; /* ids strictly ascending, in each of the three lists */
    uint32_t n_materials;
    const mi355pt_light_edit* lights;
    uint32_t n_lights;
    const mi355pt_env_edit* envs;
    uint32_t n_envs;
} mi355pt_scene_edits;
typedef struct mi355pt_edit_result {
    uint32_t rebuilt, reason, launches;
    uint32_t features_before, features_after; /* the feature bits the kernel selector reads (mi355pt_scene_info's features=) */
    double host_ms, device_ms;
} mi355pt_edit_result;

/* Replaces the descriptions of the listed materials, delta lights and environment lights of a built scene and brings the device records up
 * to date in place.  `cam` is the camera the scene is at (its position must be the built / last moved one).  Synchronous on the null
 * stream; allocates nothing on the device.  Falls back to mi355pt_scene_build of the edited description (rebuilt = 1, reason says why);
 * after MI355PT_OK the host description holds the edited records in every case.
 * Refused before anything touches the device or the description: MI355PT_E_INVALID for null arguments or three counts of 0, an id out of
 * range or ids not strictly ascending, a descriptor mi355pt_scene_add_material / mi355pt_scene_add_delta_light would refuse (the same
 * checks, the same messages), a texture or LUT id that did not exist at the build, a non-finite value, a singular light matrix, a camera
 * position other than the scene's, a scene built with mi355pt_scene_build_multi; MI355PT_E_NOT_BUILT for an unbuilt scene;
 * MI355PT_E_DEVICE when the current HIP device is not the one the scene was built on.  MI355PT_E_DEVICE on a HIP error — after which the
 * scene must be built again. */
int mi355pt_scene_edit(mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_scene_edits* e, mi355pt_edit_result* out /* NULL ok */);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_EDIT_H */
