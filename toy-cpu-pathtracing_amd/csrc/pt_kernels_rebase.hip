// Moving the camera of a built scene (include/mi355pt_rebase.h): the three kernels that recompute what a translation changes from what the
// device already holds.  Hand-written for gfx950; every one is a streaming kernel of independent threads — no LDS, no float atomics, no
// waiting between workgroups.  The arithmetic is rebase_plan.hpp's, the same functions the host refit calls, compiled without contraction
// (Makefile): the results are held to bytes against the host lowering (tests/test_rebase_gpu.py).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "rebase_plan.hpp"

namespace pt {
namespace {

constexpr uint32_t RB_BLOCK = 256;                                    // 4 waves

// 1. One thread per leaf-order triangle.  Reads the local record (3 x 16 B) and its instance's forward matrix (12 floats, wave-uniform in
// all but instanced scenes), writes the 36 position bytes of the render record; instance, flags and mclass stay.  xform_point's operation
// order (scene_lower.cpp): ((m0 x + m4 y) + m8 z) + m12, one rounding per operation.
// count_degenerate: degenerate() of the lowering on the new vertices; the wave adds its count with ONE atomic (ballot + popcount).
__global__ __launch_bounds__(RB_BLOCK) void rebase_tris_kernel(const DevTriLocal* __restrict__ local, const DevInstance* __restrict__ instances,
                                                               DevTri* __restrict__ render, uint32_t n, uint32_t count_degenerate,
                                                               uint32_t* __restrict__ degenerate_count) {
    const uint32_t i = blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool active = i < n;
    bool deg = false;
    if (active) {
        const float4* lp = reinterpret_cast<const float4*>(local + i);
        const float4 a = lp[0], b = lp[1], c = lp[2];                 // p0 p1x | p1yz p2xy | p2z instance flags mclass
        const float* m = instances[__float_as_uint(c.y)].m;
        const float px[3] = {a.x, a.w, b.z}, py[3] = {a.y, b.x, b.w}, pz[3] = {a.z, b.y, c.x};
        float q[3][3];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float s = m[r] * px[v];
                s = s + m[3 + r] * py[v];
                s = s + m[6 + r] * pz[v];
                s = s + m[9 + r];
                q[v][r] = s;
            }
        float4* rp = reinterpret_cast<float4*>(render + i);
        rp[0] = make_float4(q[0][0], q[0][1], q[0][2], q[1][0]);
        rp[1] = make_float4(q[1][1], q[1][2], q[2][0], q[2][1]);
        render[i].p2z = q[2][2];
        if (count_degenerate) {                                       // cross(b - a, c - a), dot(cr, cr) == 0: scene_lower.cpp degenerate()
            const float e1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]}, e2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
            const float cx = e1[1] * e2[2] - e2[1] * e1[2], cy = e1[2] * e2[0] - e2[2] * e1[0], cz = e1[0] * e2[1] - e2[0] * e1[1];
            deg = ((cx * cx) + (cy * cy)) + (cz * cz) == 0.0f;
        }
    }
    if (count_degenerate) {                                           // wave-uniform: every lane of the wave takes the ballot
        const unsigned long long mask = __ballot(deg);
        if (mask && (threadIdx.x & 63u) == 0u) atomicAdd(degenerate_count, (uint32_t)__popcll(mask));
    }
}

// 2. One thread per used (node, side) of ONE height group (rebase_plan.hpp): a leaf child's box from its 1 .. MAX_LEAF_TRIS triangles, a
// node child's as the union of that node's two child boxes, which the launch of a lower height wrote.  Launched lowest height first on one
// stream: the kernel boundary orders the levels.  The two sides of a node write disjoint floats of its record.
__global__ __launch_bounds__(RB_BLOCK) void refit_bvh2_kernel(DevNode* nodes, const DevTri* __restrict__ tris, const uint32_t* __restrict__ entries,
                                                              uint32_t count) {
    const uint32_t k = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= count) return;
    const uint32_t e = entries[k];
    DevNode& nd = nodes[e >> 1];
    const int side = (int)(e & 1u);
    float lo[3], hi[3];
    refit_child_box(nodes, tris, nd.child[side], lo, hi);
    store_child_box(nd, side, lo, hi);
}

// 3. One thread per child slot of the 4-wide tree: the box of its source (node, side) in the refit BVH2, padded by NODE4_PAD_REL x the
// largest coordinate magnitude of the root record's child boxes (rebase_plan.hpp pad_radius = pad_nodes4's r).  Unused slots are not touched.
__global__ __launch_bounds__(RB_BLOCK) void refit_nodes4_kernel(DevNode4* __restrict__ nodes4, const DevNode* __restrict__ nodes, const uint32_t* __restrict__ slot_src,
                                                                uint32_t n_slots, int32_t root) {
    const uint32_t k = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= n_slots) return;
    const uint32_t e = slot_src[k];
    if (e == REBASE_NO_SOURCE) return;
#if PT_NODE_FMA
    const float pad = pad_radius(nodes[root]) * NODE4_PAD_REL;
#else
    const float pad = 0.0f;
#endif
    store_slot_box(nodes4[k >> 2], (int)(k & 3u), nodes[e >> 1], (int)(e & 1u), pad);
}

inline dim3 blocks_for(uint32_t n) { return dim3((n + RB_BLOCK - 1u) / RB_BLOCK); }

}  // namespace

// ---- host side (declared in launch.hpp; called from scene_update.cpp) ----
hipError_t launch_rebase_tris(const DevTriLocal* d_local, const DevInstance* d_instances, DevTri* d_render, uint32_t n_tris, bool count_degenerate,
                              uint32_t* d_degenerate_count, hipStream_t stream) {
    if (n_tris == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rebase_tris_kernel, blocks_for(n_tris), dim3(RB_BLOCK), 0, stream, d_local, d_instances, d_render, n_tris, count_degenerate ? 1u : 0u,
                       d_degenerate_count);
    return hipGetLastError();
}
hipError_t launch_refit_bvh2_height(DevNode* d_nodes, const DevTri* d_tris_render, const uint32_t* d_entries, uint32_t first, uint32_t count, hipStream_t stream) {
    if (count == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refit_bvh2_kernel, blocks_for(count), dim3(RB_BLOCK), 0, stream, d_nodes, d_tris_render, d_entries + first, count);
    return hipGetLastError();
}
hipError_t launch_refit_nodes4(DevNode4* d_nodes4, const DevNode* d_nodes, const uint32_t* d_slot_src, uint32_t n_slots, int32_t root, hipStream_t stream) {
    if (n_slots == 0 || root < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refit_nodes4_kernel, blocks_for(n_slots), dim3(RB_BLOCK), 0, stream, d_nodes4, d_nodes, d_slot_src, n_slots, root);
    return hipGetLastError();
}

}  // namespace pt
