// Editing materials of a built scene (include/mi355pt_edit.h): the one kernel an edit can need — the rest of it is uploads into the
// existing allocations (scene_update.cpp).  Hand-written for gfx950: a streaming kernel of independent threads — no LDS, no atomics, no
// waiting between workgroups — that only MOVES a word from the table the host laid out (scene_edit_plan.hpp edit_class_table) into the
// triangle records; no arithmetic on a value, so the records are the host lowering's by construction (tests/test_scene_edit_gpu.py holds
// them to its digests).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "scene_edit_plan.hpp"

namespace pt {
namespace {

constexpr uint32_t RC_BLOCK = 256;                                    // 4 waves

// One thread per leaf-order triangle.  Reads the material word of the shading record and that material's word of the table; a triangle
// whose material keeps its class ends there, nothing written.  Otherwise the class goes into the last word of the triangle's record in
// every array that holds one: the local records, the render-space records and — where it is neither of the two — the array the traversals read.
__global__ __launch_bounds__(RC_BLOCK) void reclass_tris_kernel(DevTriLocal* __restrict__ local, DevTri* __restrict__ render, DevTri* __restrict__ walked,
                                                                const DevTriShade* __restrict__ shade, const uint32_t* __restrict__ table, uint32_t n,
                                                                uint32_t n_materials) {
    const uint32_t i = blockIdx.x * RC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t mat = shade[i].material;
    if (mat >= n_materials) return;                                   // (never: the lowering wrote the index)
    const uint32_t cls = table[mat];
    if (cls == EDIT_CLASS_UNCHANGED) return;
    local[i].mclass = cls;
    render[i].mclass = cls;
    if (walked) walked[i].mclass = cls;
}

}  // namespace

// ---- host side (declared in launch.hpp; called from scene_update.cpp) ----
hipError_t launch_reclass_tris(DevTriLocal* d_local, DevTri* d_render, DevTri* d_walked, const DevTriShade* d_shade, const uint32_t* d_table, uint32_t n_tris,
                               uint32_t n_materials, hipStream_t stream) {
    if (n_tris == 0 || n_materials == 0 || !d_local || !d_render || !d_shade || !d_table) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reclass_tris_kernel, dim3((n_tris + RC_BLOCK - 1u) / RC_BLOCK), dim3(RC_BLOCK), 0, stream, d_local, d_render, d_walked, d_shade, d_table, n_tris,
                       n_materials);
    return hipGetLastError();
}

}  // namespace pt
