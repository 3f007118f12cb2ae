// The device side of a scene: SceneImpl::build drives the lowering (scene_lower.cpp, pure host code) around the tree build and uploads
// what it produced.  Host-only C++ (compiled by hipcc).
#include "scene.hpp"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "path_end_plan.hpp"
#include "scene_lower.hpp"

namespace pt {

namespace {

template <typename T>
int upload_array(SceneImpl* s, const std::vector<T>& v, const T** out, std::string* err) {
    void* p = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { *err = std::string("hipMalloc: ") + hipGetErrorString(e); return MI355PT_E_DEVICE; }
    s->allocs.push_back(p);
    if (!v.empty()) {
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) { *err = std::string("hipMemcpy: ") + hipGetErrorString(e); return MI355PT_E_DEVICE; }
    }
    *out = (const T*)p;
    return MI355PT_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

SceneImpl::~SceneImpl() { release(); }
void SceneImpl::release() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    rebase = RebaseState{};
    built = false;
}

// The one place that allocates and copies: every array of `ls`, then `dev` with the device pointers in place of the null ones.
int SceneImpl::upload(const LoweredScene& ls, std::string* err) {
    int rc;
    dev = ls.dev;
    if ((rc = upload_array(this, ls.nodes, &dev.nodes, err))) return rc;
#if PT_NODE_Q16
    if ((rc = upload_array(this, ls.nodes4, &dev.nodes4q, err))) return rc;
#else
    if ((rc = upload_array(this, ls.nodes4, &dev.nodes4, err))) return rc;
#endif
    if ((rc = upload_array(this, ls.tris_render, &dev.tris_render, err))) return rc;
    if ((rc = upload_array(this, ls.shade, &dev.shade, err))) return rc;
    if ((rc = upload_array(this, ls.instances, &dev.instances, err))) return rc;
    if ((rc = upload_array(this, ls.tris_local, &dev.tris_local, err))) return rc;
    dev.tris = dev.tris_are_local ? dev.tris_local : dev.tris_render;
    if ((rc = upload_array(this, ls.cc_albedo, &dev.cc_albedo, err))) return rc;
    if ((rc = upload_array(this, ls.materials, &dev.materials, err))) return rc;
    {   // the light records, and behind them one box record per light (path_end_plan.hpp light_boxes: what a doomed path's ray is tested against)
        const std::vector<unsigned char> bytes = light_allocation(ls.lights, ls.light_tris, ls.dev.tri_shift);
        const unsigned char* p = nullptr;
        if ((rc = upload_array(this, bytes, &p, err))) return rc;
        dev.lights = (const DevLight*)p;
    }
    if ((rc = upload_array(this, ls.light_tris, &dev.light_tris, err))) return rc;
    if ((rc = upload_array(this, ls.light_uvs, &dev.light_uvs, err))) return rc;
    if ((rc = upload_array(this, ls.luts, &dev.luts, err))) return rc;
    if ((rc = upload_array(this, ls.cmf, &dev.cmf, err))) return rc;
    if ((rc = upload_array(this, ls.rgb2spec, &dev.rgb2spec, err))) return rc;
    if ((rc = upload_array(this, ls.z_nodes, &dev.z_nodes, err))) return rc;
    if ((rc = upload_array(this, ls.texels, &dev.texels, err))) return rc;
    if ((rc = upload_array(this, ls.textures, &dev.textures, err))) return rc;
    std::vector<DevEnv> envs = ls.envs;                    // each record names its three tables on the device
    for (size_t ek = 0; ek < envs.size(); ++ek) {
        if ((rc = upload_array(this, ls.env_tables[ek].texels, &envs[ek].texels, err))) return rc;
        if ((rc = upload_array(this, ls.env_tables[ek].marginal, &envs[ek].marginal, err))) return rc;
        if ((rc = upload_array(this, ls.env_tables[ek].conditional, &envs[ek].conditional, err))) return rc;
    }
    return upload_array(this, envs, &dev.envs, err);
}

int SceneImpl::build(const mi355pt_camera* cam, const float* cmf4 /*470*4*/, std::string* err) {
    release();
    int ndev = 0, rc;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { *err = "no HIP device: the product path requires a gfx950 GPU"; return MI355PT_E_NO_DEVICE; }
    (void)hipGetDevice(&device);
    std::memcpy(build_cam_pos, cam->position, sizeof(build_cam_pos));

    LoweredGeometry geo;
    if ((rc = lower_geometry(*this, cam, &geo, err))) return rc;

    // BVH: host sweep SAH, or the GPU binned-SAH builder for large triangle counts
    BvhOut bvh;
    double ms[3] = {0.0, 0.0, 0.0};               // bvh_ms (wall time of the tree build), bvh_device_ms (the device part of a GPU build), collapse_ms
    bool gpu_built = false;
    {
        int mode = bvh_builder;
        if (const char* e = getenv("MI355PT_BVH_BUILDER")) {
            if (!strcmp(e, "host")) mode = MI355PT_BVH_HOST; else if (!strcmp(e, "gpu")) mode = MI355PT_BVH_GPU; else if (!strcmp(e, "auto")) mode = MI355PT_BVH_AUTO;
        }
        const bool want_gpu = mode == MI355PT_BVH_GPU || (mode == MI355PT_BVH_AUTO && geo.build_tris.size() >= BVH_GPU_AUTO_TRIS);
        const auto t0 = std::chrono::steady_clock::now();
        if (want_gpu) {
            std::string why;
            gpu_built = build_bvh_gpu(geo.build_tris, &bvh, &ms[1], &why);
            if (!gpu_built && mode == MI355PT_BVH_GPU) { *err = why; return MI355PT_E_DEVICE; }   // asked for explicitly: no silent substitute
        }
        if (!gpu_built) build_bvh(geo.build_tris, &bvh);
        ms[0] = ms_since(t0);
    }
    if (bvh.max_depth >= STACK_DEPTH) { *err = "BVH deeper than the traversal stack"; return MI355PT_E_INVALID; }

    RebaseState rb;                                 // what a later move (of the camera, of instances) needs of the build's intermediate results
    keep_topology(geo, bvh, cam, gpu_built, &rb);

    LoweredScene ls;
    LowerReport rep;
    if ((rc = lower_scene(*this, std::move(geo), std::move(bvh), cmf4, &ls, &rep, err))) return rc;
    const auto tc = std::chrono::steady_clock::now();
    if ((rc = lower_tree4(&ls, &rep, err))) return rc;
    ms[2] = ms_since(tc);

    if ((rc = upload(ls, err))) return rc;
    rebase = std::move(rb);
    if ((rc = prepare_rebase(ls, rep, err))) return rc;
    features = ls.features;
    info = lowering_info(ls, rep, gpu_built, ms);
    built = true;
    return MI355PT_OK;
}

}  // namespace pt
