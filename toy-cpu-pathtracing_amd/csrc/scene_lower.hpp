// Scene lowering, the part that needs no device: description + camera -> the host arrays SceneImpl::build uploads (layout.hpp).
// Host-only and pure: no HIP header, no environment variable, no clock — the same description gives the same bytes, on any machine
// with the same libm (tests/test_scene_lowering.py holds the digests).  Two stages around the BVH2 build, which the caller owns:
//
//   lower_geometry   description + camera -> records in creation order, the builder's input       (stage A)
//   [ build_bvh / build_bvh_gpu: scene.cpp picks one ]
//   lower_scene      geometry + BVH2      -> everything in leaf order, every table and scalar      (stage B)
//   lower_tree4      ... and the 4-wide tree the traversals walk; a call of its own so that the caller can time the collapse
#pragma once
#include <array>
#include <string>
#include <vector>

#include "scene.hpp"

namespace pt {

// Stage A's result.  Triangle records are in creation order (instance by instance); build_tris / kept leave out the degenerate ones.
struct LoweredGeometry {
    std::vector<DevInstance> instances;
    std::vector<DevTri> tris;                  // render-space vertices
    std::vector<DevTriLocal> tris_local;       // the mesh's own vertices
    std::vector<DevTriShade> shade;
    std::vector<BuildTri> build_tris;          // bounds of the triangles the tree is built over
    std::vector<uint32_t> kept;                // build index -> triangle
    size_t n_degenerate = 0;                   // triangles with an exactly zero cross product: never hit (ray.rs:49-56), left out of the tree
    std::vector<DevLight> lights;              // area lights and delta / environment lights, in creation order
    std::vector<DevLightTri> light_tris;
    std::vector<float> light_uvs;              // 6 per light triangle (original vertex order), zeros without texcoords
    std::vector<uint32_t> env_light_index;     // position of environment light k in the light list
    std::vector<std::array<float, 16>> env_l2r;
    bool tris_are_local = false;               // every instance is the same pure translation: the traversals test the local vertices
    float shared_iw[3] = {0, 0, 0}, shared_mw[3] = {0, 0, 0};   // that translation's inverse / forward offsets
};

// Everything SceneImpl::upload needs and nothing else: the arrays in upload order, then what DevScene holds besides pointers.
struct LoweredScene {
    std::vector<DevNode> nodes;
#if PT_NODE_Q16
    std::vector<DevNode4Q> nodes4;
#else
    std::vector<DevNode4> nodes4;
#endif
    std::vector<DevTri> tris_render;
    std::vector<DevTriShade> shade;
    std::vector<DevInstance> instances;
    std::vector<DevTriLocal> tris_local;
    std::vector<float> cc_albedo;
    std::vector<DevMaterial> materials;        // the device copy: texture descriptors, clearcoat table offsets, the environment lights' spectra
    std::vector<DevLight> lights;
    std::vector<DevLightTri> light_tris;
    std::vector<float> light_uvs, luts, cmf, rgb2spec, z_nodes;
    std::vector<uint32_t> texels;
    std::vector<DevTexture> textures;
    struct EnvTables { std::vector<float> texels, marginal, conditional; };
    std::vector<EnvTables> env_tables;
    std::vector<DevEnv> envs;                  // the three pointers of each are null: upload fills them in
    DevScene dev{};                            // every non-pointer field; the pointers are null
    uint32_t features = 0;                     // FEAT_* bits the scene needs (kernel specialisation)
};

// What lowering found out along the way: scene_info's numbers that are not in DevScene.
struct LowerReport {
    size_t n_degenerate = 0;
    int bvh_depth = 0;
    int stack_need = 0;                        // worst-case per-lane stack entries the collapsed tree can need (< STACK_DEPTH, validated)
    const char* collapse_method = "";          // "dp" or "greedy"
};

// Stage A.  Errors (MI355PT_E_INVALID): "scene has no instances", "singular instance transform", "scene has no triangles", "too many triangles".
int lower_geometry(const SceneImpl& scene, const mi355pt_camera* cam, LoweredGeometry* out, std::string* err);
// Stage B.  Consumes the geometry and the tree (their arrays move into *out); cmf4: [470][4].
int lower_scene(const SceneImpl& scene, LoweredGeometry&& geo, BvhOut&& bvh, const float* cmf4, LoweredScene* out, LowerReport* rep, std::string* err);
int lower_tree4(LoweredScene* ls, LowerReport* rep, std::string* err);   // ls->nodes -> ls->nodes4 (+ root4, n_nodes4, the Q16 grid)
float nodes4_pad_radius(const std::vector<DevNode4>& nodes4);   // r of the pad lower_tree4 applies (PT_NODE_FMA): largest |coordinate| over the used slots, BEFORE the pad

// What a camera TRANSLATION changes besides the triangles' positions and the boxes of the two trees (mi355pt_scene_move_camera,
// scene_rebase.cpp): lower_geometry's own functions on the instance matrices, the delta lights, the scene bounds (from the meshes' local
// boxes, which the caller caches: mesh_local_bounds) and the emissive triangles.  `built_lights` / `built_light_tris`: the records of the
// build — an area light's record and a light triangle's cdf hold world-space areas and stay.
void mesh_local_bounds(const SceneImpl& scene, std::vector<MeshBounds>* out);
struct CameraRecords {
    std::vector<DevInstance> instances;
    std::vector<DevLight> lights;
    std::vector<DevLightTri> light_tris;
    bool tris_are_local = false;
    float shared_iw[3] = {0, 0, 0}, shared_mw[3] = {0, 0, 0};
    std::vector<uint32_t> env_light_index;     // as in LoweredGeometry: what lower_environment takes beside the description
    std::vector<std::array<float, 16>> env_l2r;
};
int lower_camera_records(const SceneImpl& scene, const mi355pt_camera* cam, const std::vector<MeshBounds>& bounds, const std::vector<DevLight>& built_lights,
                         const std::vector<DevLightTri>& built_light_tris, CameraRecords* out, std::string* err, const uint8_t* moved = nullptr,
                         std::vector<float>* light_pdf = nullptr);
// ... and what NEW local_to_world matrices change besides (mi355pt_scene_move_instances, scene_instances.cpp): `moved` (per instance, NULL =
// none) marks the instances whose matrix differs from the one `built_lights` / `built_light_tris` were made for.  A moved emissive instance
// gets its world-space area tables again (area_light_tables on the description's matrix): DevLight::area_sum, every DevLightTri::cdf, and in
// *light_pdf (NULL ok; one float per light triangle, indexed DevLight::first_tri + triangle, 0 for unmoved lights) DevTriShade::light_pdf_area.
// `lowering`'s test of a matrix (finite, not singular; the whole instance record) on its own: false = mi355pt_scene_build would refuse it
bool instance_transform_ok(const SceneImpl& scene, const mi355pt_camera* cam, const float* l2w);
// What a later move keeps of stage A and the tree build (RebaseState, scene.hpp): the tree as its builder returned it, the camera position it
// was built for, the triangles it leaves out
void keep_topology(const LoweredGeometry& geo, const BvhOut& bvh, const mi355pt_camera* cam, bool gpu_built, RebaseState* rb);
// degenerate() on the render-space vertices of triangle `tri` of instance `instance`, whose lowered record is `di`
bool render_triangle_degenerate(const SceneImpl& scene, const DevInstance& di, uint32_t instance, uint32_t tri);
// The host gates of an update in place.  Same lowering class: `instances` / `tris_are_local` have the classes `identity` (DevInstance::identity
// per instance) / `built_local` name.  Every triangle the built tree leaves out (RebaseState::left_out) is still degenerate; with `moved`, of the marked instances only
bool same_lowering_class(const std::vector<DevInstance>& instances, bool tris_are_local, const std::vector<uint8_t>& identity, bool built_local);
bool left_out_stay_degenerate(const SceneImpl& scene, const std::vector<DevInstance>& instances, const uint8_t* moved = nullptr);

// What NEW VERTICES of a mesh change besides (mi355pt_scene_deform_meshes, scene_deform.cpp): one mesh's entry of mesh_local_bounds again,
// and degenerate() on the LOCAL vertices of triangle `tri` of a mesh — the set the tree leaves out in local-triangle mode.  With the
// instances of the deformed meshes marked in `moved`, lower_camera_records gives an emissive one its area tables from the new vertices
void mesh_local_bounds_of(const SceneImpl& scene, uint32_t geom, MeshBounds* out);
bool local_triangle_degenerate(const HostMesh& mesh, uint32_t tri);

// What NEW DESCRIPTIONS of materials, delta lights and environment lights change (mi355pt_scene_edit, scene_edit.cpp), for a description
// whose emitter set and clearcoat count are the build's: the device copy of the materials and the coat-albedo table (finish_materials; a
// clearcoat material not marked in `material_changed` keeps the row `built` holds), the light list (lower_camera_records: lower_delta_light
// with set_directional_areas over the cached mesh bounds), for every environment marked in `env_edited` its record, its tables and the
// integrated spectrum of its hidden material (lower_environment; the others keep the records of `built`), and scene_features
struct EditMaterialKey;   // scene_edit_plan.hpp
struct EditRecords {
    std::vector<DevMaterial> materials;
    std::vector<float> cc_albedo;
    std::vector<DevLight> lights;
    std::vector<DevEnv> envs;                                // the three pointers of each are null
    std::vector<LoweredScene::EnvTables> env_tables;         // of the marked environments; the others' stay empty
    uint32_t features = 0;
};
int lower_edit_records(const SceneImpl& scene, const mi355pt_camera* cam, const RebaseState& built, const uint8_t* material_changed, const uint8_t* env_edited,
                       EditRecords* out, std::string* err);
void material_keys(const std::vector<DevMaterial>& materials, std::vector<EditMaterialKey>* out);   // what scene_edit_plan.hpp reads of each record

// scene_info's text; ms = {bvh_ms, bvh_device_ms, collapse_ms} or null to leave the three timings out (what the digests are recorded with)
std::string lowering_info(const LoweredScene& ls, const LowerReport& rep, bool gpu_builder, const double* ms);

// FNV-1a-64 of every array of `ls` in upload order, then of the scalars (DevScene's non-pointer fields, features, the report); names[i] names digests[i].
void lowering_digests(const LoweredScene& ls, const LowerReport& rep, std::vector<std::string>* names, std::vector<uint64_t>* digests);

}  // namespace pt
