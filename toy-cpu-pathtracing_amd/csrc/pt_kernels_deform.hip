// Deforming meshes of a built scene (include/mi355pt_deform.h): the one kernel the deformation puts in front of the instance move's
// sequence (pt_kernels_rebase.hip re-transforms the positions and refits both trees, pt_kernels_instances.hip refreshes ng and the light
// pdf and sums the SAH cost — whatever changed the local records).  Hand-written for gfx950: a streaming kernel of independent threads —
// no LDS, no atomics, no waiting between workgroups — that only MOVES bytes from the staging buffer the host laid out (deform_plan.hpp)
// into the local records; no arithmetic on a value, so nothing depends on contraction flags and the records are the host lowering's by
// construction (tests/test_deform_gpu.py holds them to its digests).
#include <hip/hip_runtime.h>

#include "deform_plan.hpp"
#include "launch.hpp"

namespace pt {
namespace {

constexpr uint32_t DF_BLOCK = 256;                                    // 4 waves

// One thread per leaf-order triangle.  Reads rows 4 and 5 of the shading record (uv2 material INSTANCE | flags light LOCAL_TRI
// light_pdf_area) and the instance's word of the table; a triangle whose mesh is not updated ends there, nothing written.  Otherwise the
// mesh's slot record (2 x 16 B, wave-uniform in all but instanced scenes), the triangle's three indices, the three positions and, where the
// slot names them, the three normals and the tangent.  Writes the 36 position bytes of local[i] — instance, flags and mclass go back as
// read — and, where normals or a tangent came, rows 0 - 2 of shade[i] with the words that did not come as read.
__global__ __launch_bounds__(DF_BLOCK) void deform_tris_kernel(DevTriLocal* __restrict__ local, DevTriShade* __restrict__ shade, const uint32_t* __restrict__ table,
                                                               const float* __restrict__ staging, const uint32_t* __restrict__ mesh_idx, uint32_t n,
                                                               uint32_t n_instances, uint32_t slots_at, uint32_t n_slots) {
    const uint32_t i = blockIdx.x * DF_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4* rec = reinterpret_cast<float4*>(shade + i);
    const uint32_t inst = __float_as_uint(rec[4].w), local_tri = __float_as_uint(rec[5].z);
    if (inst >= n_instances) return;                                  // (never: the lowering wrote the index)
    const uint32_t slot = table[inst];
    if (slot >= n_slots) return;                                      // DEFORM_NO_SLOT: another mesh
    const uint4* sp = reinterpret_cast<const uint4*>(table + slots_at + slot * DEFORM_SLOT_WORDS);
    const uint4 s0 = sp[0], s1 = sp[1];                               // pos nrm tangent idx | n_tri n_vert pad pad
    if (local_tri >= s1.x) return;                                    // (never: the plan was made for this mesh)
    const uint32_t* ix = mesh_idx + s0.w + 3u * local_tri;
    const uint32_t v0 = ix[0], v1 = ix[1], v2 = ix[2];
    if (v0 >= s1.y || v1 >= s1.y || v2 >= s1.y) return;               // (never: mi355pt_scene_add_mesh checked the indices)
    const float* p = staging + s0.x;
    float4* lp = reinterpret_cast<float4*>(local + i);
    const float4 c = lp[2];                                           // p2z instance flags mclass
    lp[0] = make_float4(p[3u * v0], p[3u * v0 + 1u], p[3u * v0 + 2u], p[3u * v1]);
    lp[1] = make_float4(p[3u * v1 + 1u], p[3u * v1 + 2u], p[3u * v2], p[3u * v2 + 1u]);
    lp[2] = make_float4(p[3u * v2 + 2u], c.y, c.z, c.w);
    const bool has_nrm = s0.y != DEFORM_NO_SLOT, has_tangent = s0.z != DEFORM_NO_SLOT;
    if (!has_nrm && !has_tangent) return;
    float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];                     // n0 n1x | n1yz n2xy | n2z tangent
    if (has_nrm) {
        const float* q = staging + s0.y;
        r0 = make_float4(q[3u * v0], q[3u * v0 + 1u], q[3u * v0 + 2u], q[3u * v1]);
        r1 = make_float4(q[3u * v1 + 1u], q[3u * v1 + 2u], q[3u * v2], q[3u * v2 + 1u]);
        r2.x = q[3u * v2 + 2u];
    }
    if (has_tangent) {
        const float* t = staging + s0.z + 3u * local_tri;
        r2.y = t[0]; r2.z = t[1]; r2.w = t[2];
    }
    rec[0] = r0; rec[1] = r1; rec[2] = r2;
}

}  // namespace

// ---- host side (declared in launch.hpp; called from scene_update.cpp) ----
hipError_t launch_deform_tris(DevTriLocal* d_local, DevTriShade* d_shade, const uint32_t* d_table, const float* d_staging, const uint32_t* d_mesh_idx, uint32_t n_tris,
                              uint32_t n_instances, uint32_t slots_at, uint32_t n_slots, hipStream_t stream) {
    if (n_tris == 0 || n_instances == 0 || n_slots == 0 || (slots_at & 3u) != 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deform_tris_kernel, dim3((n_tris + DF_BLOCK - 1u) / DF_BLOCK), dim3(DF_BLOCK), 0, stream, d_local, d_shade, d_table, d_staging, d_mesh_idx, n_tris,
                       n_instances, slots_at, n_slots);
    return hipGetLastError();
}

}  // namespace pt
