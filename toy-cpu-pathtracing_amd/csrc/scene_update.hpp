// The one device step (scene_update.cpp) behind the three in-place updates of a built scene: mi355pt_scene_move_camera
// (scene_rebase.cpp), mi355pt_scene_move_instances (scene_instances.cpp), mi355pt_scene_deform_meshes (scene_deform.cpp) — and, as a stage of
// its own that touches no geometry, behind mi355pt_scene_edit (scene_edit.cpp).  An entry point keeps its
// checks, the description, the host records and the host gates; everything that touches the device after them is the step's.  Not installed, not an ABI.
#pragma once
#include "api_internal.hpp"
#include "deform_plan.hpp"
#include "scene_lower.hpp"

namespace pt {

// the leading stage of a deformation: the call's arrays in deform_plan.hpp's layout and what the buffers of every later call must hold
struct DeformStage {
    const std::vector<float>& staging;
    const std::vector<uint32_t>& table;         // deform_table(plan)
    uint32_t n_slots;                           // plan.slots.size()
    const std::vector<DeformUpdate>& meshes;    // the updated meshes: the index buffer of each goes up once per build
    size_t staging_capacity, table_capacity;    // in floats / words, for every mesh of the scene at once
};

// an edit of materials and lights (scene_edit.cpp) in place of the geometry stages: the arrays that differ from the built ones (nullptr =
// as built, not uploaded), each of the built array's size, and the class table when a material changed class.  With this stage the step
// uploads and launches nothing else: no triangle position, no box and no instance record changes
struct EditStage {
    const std::vector<DevMaterial>* materials = nullptr;
    const std::vector<float>* cc_albedo = nullptr;
    const std::vector<DevLight>* lights = nullptr;
    const std::vector<DevEnv>* envs = nullptr;                               // the records without their pointers, which the step keeps
    const std::vector<LoweredScene::EnvTables>* env_tables = nullptr;        // with env_map_changed: the tables of the marked environments
    const uint8_t* env_map_changed = nullptr;                                // per environment, with envs
    const std::vector<uint32_t>* class_table = nullptr;                      // scene_edit_plan.hpp edit_class_table; nullptr: no class changed, no launch
};

struct SceneUpdate {
    const CameraRecords& rec;                   // uploaded into the existing allocations
    bool count_degenerate;                      // launch_rebase_tris counts the triangles that became degenerate
    const uint8_t* moved = nullptr;             // per instance; null: no shading record changes and the cached light records stay (the camera move)
    const std::vector<float>* light_pdf = nullptr;   // with `moved`: light_pdf_area per light triangle
    bool sah = false;                           // take sah_built (once per build, ahead of everything) and sah_after, compare with rebuild_above
    float rebuild_above = 0.0f;
    const DeformStage* deform = nullptr;
    const EditStage* edit = nullptr;            // with it, `rec` and everything above are not read
};

struct SceneUpdateResult {
    // DEGENERATE_SET_CHANGED, SAH_DEGRADED: the launches ran; the caller builds again, which overwrites everything they wrote.  DEVICE_ERROR:
    // a HIP error, `what` names it ("hipMemcpy: <hipGetErrorString>"); the scene has been dropped (SceneImpl::release)
    enum Outcome { DONE, DEGENERATE_SET_CHANGED, SAH_DEGRADED, DEVICE_ERROR } outcome = DONE;
    uint32_t launches = 0;
    double device_ms = 0.0;                     // HIP-event time from the first launch to the last
    float sah_built = 0.0f, sah_after = 0.0f;   // with SceneUpdate::sah, after DONE
    std::string what;
};

// On the null stream, synchronous.  The scene is built and rebase.ready (a build with quantised 4-wide nodes never is)
SceneUpdateResult scene_update_step(SceneImpl* impl, const SceneUpdate& u);

}  // namespace pt
