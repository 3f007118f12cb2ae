// Host-side scene: stores what the C ABI hands over, lowers it to the flat HBM layout of layout.hpp
// (single render-space BVH over all instances, leaf-ordered triangles, per-triangle shading records,
// light tables) and owns the device buffers.  Replaces Scene::build (scene/src/scene.rs:64-76).
// The lowering itself is scene_lower.hpp (pure host code); scene.cpp is what needs a device.
#pragma once
#include <string>
#include <vector>

#include "../../include/mi355pt.h"
#include "layout.hpp"

namespace pt {

struct HostMesh {
    std::vector<float> pos, nrm, uv, tangent;   // nrm normalised twice like Normal::new (normal.rs:18-20,93-100)
    std::vector<uint32_t> idx;
    uint32_t n_vert = 0, n_tri = 0;
};
struct HostInstance { uint32_t geom, mat; float l2w[16]; uint32_t dynamic = 0; };   // dynamic: mi355pt_scene_set_instance_dynamic (include/mi355pt_instances.h)
struct HostDeltaLight { mi355pt_light_desc d; uint32_t material; uint32_t after_instances; uint32_t env_index = 0; };   // hidden emissive material holds the spectrum

struct BuildTri { float lo[3], hi[3], c[3]; };
struct BvhOut {
    std::vector<DevNode> nodes;
    std::vector<uint32_t> order;   // leaf-ordered triangle permutation
    int32_t root = 0;
    int max_depth = 0;
};
// Sweep-SAH BVH2 over triangle bounds; children boxes stored in the parent (layout.hpp DevNode).
void build_bvh(const std::vector<BuildTri>& tris, BvhOut* out);
// BVH2 -> BVH4 for the cooperative traversals (layout.hpp DevNode4), with the stack-need guarantee validated; host only (bvh_builder.cpp)
bool collapse_bvh4(const std::vector<DevNode>& nodes2, int32_t root2, size_t n_tris, std::vector<DevNode4>* nodes4, int32_t* root4, int* max_stack,
                   std::string* err, const char** method = nullptr);   // *method: "dp" (cost-optimal) or "greedy" (above 1.2 M nodes, or no memory for the tables)
// SAH constants shared by both builders (env overrides MI355PT_BVH_COST_TRI / MI355PT_BVH_LEAF are for sweeps only)
void bvh_build_config(float* cost_traverse, float* cost_tri, int* leaf_max);
// The same contract built on the current HIP device (bvh_gpu.hip): breadth-first binned SAH, one round of launches
// per level.  Returns false with *err set when it cannot build (n < 8, out of memory, HIP error).
bool build_bvh_gpu(const std::vector<BuildTri>& tris, BvhOut* out, double* device_ms, std::string* err);

constexpr size_t BVH_GPU_AUTO_TRIS = 1u << 17;   // "auto": scenes from 131 072 triangles on are built on the GPU

struct LoweredScene;   // scene_lower.hpp
struct LowerReport;

struct MeshBounds { float lo[3], hi[3]; };   // a mesh's local AABB (scene_lower.cpp mesh_local_bounds)
// What the updates in place (scene_rebase.cpp, scene_instances.cpp, scene_deform.cpp; their device step scene_update.cpp) keep beside the lowered scene, made by SceneImpl::build.  Not part of LoweredScene: what
// the upload takes and the digests hash stays what it was.
struct RebaseState {
    bool ready = false;                       // false: a move builds again (MI355PT_MOVE_UNSUPPORTED_BUILD)
    bool pinned = false;                      // the host side tables below are there (a build, or mi355pt_scene_debug_pin_host_tree without a device)
    bool gpu_built = false;
    std::vector<uint32_t> height_offset;      // rebase_plan.hpp RebasePlan::height_offset
    uint32_t n_slots = 0;                     // 4 * n_nodes4
    uint32_t* d_entries = nullptr;            // RebasePlan::entries, RebasePlan::slot_src and the degenerate counter, on the device
    uint32_t* d_slot_src = nullptr;           // (all three in SceneImpl::allocs)
    uint32_t* d_count = nullptr;
    std::vector<uint8_t> identity;            // DevInstance::identity of the build, per instance
    bool tris_are_local = false;
    std::vector<uint32_t> left_out;           // (instance, mesh triangle) pairs the build found degenerate in render space and left out of the tree
    std::vector<MeshBounds> bounds;           // per mesh
    std::vector<DevLight> lights;             // the build's records: an area light's and a light triangle's cdf do not depend on the camera
    std::vector<DevLightTri> light_tris;
    std::vector<DevNode> tree_nodes;          // the built tree as its builder returned it, either builder's (after an instance move the host
    std::vector<uint32_t> tree_order;         // builder would no longer reproduce it from the description): what the pinned lowerings
    int tree_depth = 0; int32_t tree_root = 0;   // (mi355pt_scene_debug_move_digest for a GPU-built tree, mi355pt_scene_debug_pinned_digest) pin the topology to
    std::vector<DevNode4> tree_nodes4;        // ... and its 4-wide collapse (links and used slots; the boxes follow a refit)
    int32_t tree_root4 = 0;
    std::vector<uint32_t> kept;               // build index -> triangle of the build, when it left triangles out (else the identity, not stored)
    // mi355pt_scene_edit (scene_edit.cpp): the lowered records an edit compares with and starts from, as the build uploaded them
    std::vector<DevMaterial> materials;       // the device copy (texture descriptors, coat table offsets, the environments' integrated spectra)
    std::vector<float> cc_albedo;
    std::vector<DevTexture> textures;         // the build's textures and LUTs: an edit names no later one
    uint32_t n_luts = 0;
    std::vector<DevEnv> envs;                 // the three pointers of each are null
    uint32_t* d_class_table = nullptr;        // one word per material (in SceneImpl::allocs, made by the build)
    // mi355pt_scene_move_instances (scene_instances.cpp, scene_update.cpp): allocated / computed by the first move after a build (all in SceneImpl::allocs)
    uint32_t n_entries = 0;                   // RebasePlan::entries.size()
    float* d_sah = nullptr;                   // launch_sah_cost's scratch
    uint32_t* d_moved_bits = nullptr;         // one bit per instance
    float* d_light_pdf = nullptr;             // light_pdf_area per light triangle
    bool sah_built_valid = false;
    float sah_built = 0.0f;
    // mi355pt_scene_deform_meshes (scene_deform.cpp, scene_update.cpp): allocated by the first deformation after a build (all in SceneImpl::allocs)
    float* d_deform_staging = nullptr;        // deform_plan.hpp: the new arrays of one call, sized for every mesh of the scene at once
    uint32_t* d_deform_table = nullptr;       // ... the slot per instance and the slot records
    uint32_t* d_mesh_idx = nullptr;           // ... the index buffers of all meshes, one after the other
    std::vector<uint32_t> mesh_idx_offset;    // first word of mesh g in that pool (n_meshes + 1 entries)
    std::vector<uint8_t> mesh_idx_uploaded;   // per mesh: its indices are on the device (uploaded once per build, by its first deformation)
    // mi355pt_scene_flow_mark (api_flow.cpp): allocated by the first mark after a build (in SceneImpl::allocs).  Every build starts from a fresh
    // RebaseState (SceneImpl::release), so a build — a move's fallback included — drops the mark
    DevTri* d_tris_prev = nullptr;            // the render-space leaf-order triangles as they were when the mark was taken (n_tris records)
    bool flow_marked = false;
    float tree_cam_pos[3] = {0, 0, 0};        // the camera position the tree was BUILT for (build_cam_pos follows the moves)
    size_t n_degenerate = 0; int bvh_depth = 0, stack_need = 0; std::string collapse_method;   // the build's LowerReport (mi355pt_scene_debug_device_digest)
};

struct SceneImpl {
    // ---- description ----
    std::vector<float> table;                 // reference layout [64][3][64][64][64][3]
    std::vector<std::vector<float>> luts;
    struct Tex { std::vector<uint8_t> rgb; uint32_t w, h; };
    std::vector<Tex> textures;
    std::vector<HostMesh> meshes;
    std::vector<DevMaterial> materials;
    std::vector<HostInstance> instances;
    struct HostEnv { float intensity = 1.0f; uint32_t w = 0, h = 0, illuminant_lut = 0; std::vector<float> rgb; float l2w[16]; };
    std::vector<HostEnv> envs;                  // environment lights in creation order (HostDeltaLight::d.angle_inner carries the index)
    std::vector<HostDeltaLight> delta_lights;   // creation order; after_instances = instances.size() at creation (light_sampler.rs:163-180)
    int bvh_builder = 0;          // MI355PT_BVH_AUTO / _HOST / _GPU (mi355pt_scene_set_bvh_builder)
    int lowering = 0;             // mi355pt_scene_debug_set_lowering: 0 auto, 1 never the local triangle array, 2 also every instance through the full matrix path
    // ---- built ----
    bool built = false;
    int device = -1;              // the HIP device build() uploaded to: render calls must run with it current
    float build_cam_pos[3] = {0, 0, 0};   // camera position baked into the render-space records (world -> render translation)
    DevScene dev{};
    std::vector<void*> allocs;
    uint32_t features = FEAT_ALL;   // FEAT_* bits the scene's materials need (kernel specialisation)
    std::string info;             // mi355pt_scene_info
    RebaseState rebase;

    ~SceneImpl();
    void release();
    // RgbSigmoidPolynomial::from(ColorSrgb) on the host (rgb_sigmoid_polynomial.rs:87-155)
    bool table_lookup_srgb(const float rgb_encoded[3], float c[3], bool linear = false) const;
    int lower_spectrum(const mi355pt_spectrum& in, DevSpectrum* out, int allow_texture /* 0 no, 1 Albedo type, 2 every SpectrumType */, std::string* err) const;
    // release(), the device query, lower_geometry, the tree build (host or GPU), lower_scene + lower_tree4, upload, the info string
    int build(const mi355pt_camera* cam, const float* cmf4 /*470*4*/, std::string* err);
    int upload(const LoweredScene& ls, std::string* err);   // the one place that allocates device memory and copies to it
    // scene_rebase.cpp: the side tables of a built scene, after upload(); on_device = false: the host tables only (rebase.pinned, not .ready)
    int prepare_rebase(const LoweredScene& ls, const LowerReport& rep, std::string* err, bool on_device = true);
};

// mi355pt_coat_albedo_table (scene_lower.cpp): E(cos theta_o) of the clearcoat's directional-albedo estimator, 64 entries
void coat_albedo_table(float alpha, float r0, float out[64]);

}  // namespace pt
