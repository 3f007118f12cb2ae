// Moving instances of a built scene (include/mi355pt_instances.h): the kernels the move adds to the camera move's three
// (pt_kernels_rebase.hip re-transforms the positions and refits both trees, whatever moved them).  Hand-written for gfx950.
//   shade_refresh_kernel   the geometric normal and the light pdf of the shading records of the moved instances: independent threads,
//                          no LDS;
//   sah_terms_kernel /     the SAH cost of the refit BVH2, a fixed-order sum (instance_move_plan.hpp): SAH_BLOCK floats of LDS, no float
//   sah_finish_kernel      atomics, nothing that depends on scheduling.
// The arithmetic is instance_move_plan.hpp's, the same functions the host lowering calls, compiled without contraction (Makefile), with
// hipcc's default correctly rounded division and square root: the results are held to bytes against the host
// (tests/test_instance_move_gpu.py).
#include <hip/hip_runtime.h>

#include "instance_move_plan.hpp"
#include "launch.hpp"

namespace pt {
namespace {

constexpr uint32_t IM_BLOCK = 256;                                    // 4 waves
static_assert(IM_BLOCK == SAH_BLOCK, "one thread per lane of the reduction tree");

// 1. One thread per leaf-order shading record.  Reads the record's last three 16-byte rows (uv2 material instance | flags light local_tri
// light_pdf_area | ng pad_ng), the triangle's local vertices, its instance's inverse matrix and the instance's bit of the moved table —
// for every record, moved or not; only the light table is read under a condition (a record that is not emissive names no light).  Writes
// rows 5 and 6 of the records whose instance moved: ng recomputed (shade_normal), light_pdf_area of an emissive triangle copied from the
// uploaded table at lights[light].first_tri + local_tri; every other word goes back as it was read.
__global__ __launch_bounds__(IM_BLOCK) void shade_refresh_kernel(DevTriShade* __restrict__ shade, const DevTriLocal* __restrict__ local,
                                                                 const DevInstance* __restrict__ instances, const uint32_t* __restrict__ moved_bits,
                                                                 const DevLight* __restrict__ lights, const float* __restrict__ light_pdf, uint32_t n,
                                                                 uint32_t n_instances, uint32_t n_lights, uint32_t n_light_pdf) {
    const uint32_t i = blockIdx.x * IM_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4* rec = reinterpret_cast<float4*>(shade + i);
    const float4 r4 = rec[4], r5 = rec[5], r6 = rec[6];
    const float4* lp = reinterpret_cast<const float4*>(local + i);
    const float4 a = lp[0], b = lp[1], c = lp[2];                     // p0 p1x | p1yz p2xy | p2z instance flags mclass
    const uint32_t inst = __float_as_uint(r4.w);
    if (inst >= n_instances) return;                                  // (never: the lowering wrote the index)
    const DevInstance& di = instances[inst];
    float inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = di.inv[k];
    const bool identity = di.identity != 0u;
    const bool moved = (moved_bits[inst >> 5] >> (inst & 31u)) & 1u;
    const IV3 ng = shade_normal(IV3{a.x, a.y, a.z}, IV3{a.w, b.x, b.y}, IV3{b.z, b.w, c.x}, inv, identity);
    float pdf = r5.w;
    const uint32_t flags = __float_as_uint(r5.x), light = __float_as_uint(r5.y), local_tri = __float_as_uint(r5.z);
    if ((flags & 2u) && light < n_lights) {
        const uint32_t at = lights[light].first_tri + local_tri;
        if (at < n_light_pdf) pdf = light_pdf[at];
    }
    if (moved) {
        rec[5] = make_float4(r5.x, r5.y, r5.z, pdf);
        rec[6] = make_float4(ng.x, ng.y, ng.z, r6.w);
    }
}

// the stride-halving tree over the block's SAH_BLOCK values (instance_move_plan.hpp sah_tree_step); v[0] is the block's sum afterwards
__device__ __forceinline__ void sah_block_tree(float* v, uint32_t t) {
    for (uint32_t s = SAH_BLOCK / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) sah_tree_step(v, t, s);
    }
    __syncthreads();
}

// 2. One thread per entry of the refit plan (all height groups): its term, the block's terms summed in the tree, the block's sum to
// partial[block].  A thread past the last entry holds +0.0.
__global__ __launch_bounds__(IM_BLOCK) void sah_terms_kernel(const DevNode* __restrict__ nodes, const uint32_t* __restrict__ entries, uint32_t n_entries,
                                                             float* __restrict__ partial) {
    __shared__ float v[SAH_BLOCK];
    const uint32_t t = threadIdx.x, k = blockIdx.x * SAH_BLOCK + t;
    float term = 0.0f;
    if (k < n_entries) { const uint32_t e = entries[k]; term = sah_term(nodes[e >> 1], (int)(e & 1u)); }
    v[t] = term;
    sah_block_tree(v, t);
    if (t == 0) partial[blockIdx.x] = v[0];
}

// 3. ONE block: the block sums, summed the same way level by level in place (block c of a level reads partial[c * SAH_BLOCK ...] and writes
// partial[c], which no later block of the level reads) until one value is left; then out[0] = that sum / a(root), out[1] = the sum,
// out[2] = a(root).  The barriers of the tree order a level's stores before the next level's loads within the block.
__global__ __launch_bounds__(IM_BLOCK) void sah_finish_kernel(const DevNode* __restrict__ nodes, int32_t root, float* partial, uint32_t n_partial, float* __restrict__ out) {
    __shared__ float v[SAH_BLOCK];
    const uint32_t t = threadIdx.x;
    uint32_t count = n_partial;
    while (count > 1u) {
        const uint32_t nb = (count + SAH_BLOCK - 1u) / SAH_BLOCK;
        for (uint32_t c = 0; c < nb; ++c) {
            const uint32_t k = c * SAH_BLOCK + t;
            const float x = k < count ? partial[k] : 0.0f;
            __syncthreads();                                          // (the previous block's v[0] has been read)
            v[t] = x;
            sah_block_tree(v, t);
            if (t == 0) partial[c] = v[0];
        }
        __syncthreads();
        count = nb;
    }
    if (t == 0) {
        const float sum = partial[0], area = root_half_area(nodes[root]);
        out[0] = sah_quotient(sum, area); out[1] = sum; out[2] = area;
    }
}

inline dim3 blocks_for(uint32_t n) { return dim3((n + IM_BLOCK - 1u) / IM_BLOCK); }

}  // namespace

// ---- host side (declared in launch.hpp; called from scene_update.cpp) ----
hipError_t launch_shade_refresh(DevTriShade* d_shade, const DevTriLocal* d_local, const DevInstance* d_instances, const uint32_t* d_moved_bits, const DevLight* d_lights,
                                const float* d_light_pdf, uint32_t n_tris, uint32_t n_instances, uint32_t n_lights, uint32_t n_light_pdf, hipStream_t stream) {
    if (n_tris == 0 || n_instances == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(shade_refresh_kernel, blocks_for(n_tris), dim3(IM_BLOCK), 0, stream, d_shade, d_local, d_instances, d_moved_bits, d_lights, d_light_pdf, n_tris,
                       n_instances, n_lights, n_light_pdf);
    return hipGetLastError();
}
size_t sah_scratch_floats(uint32_t n_entries) { return (size_t)sah_blocks(n_entries) + 4; }
hipError_t launch_sah_cost(const DevNode* d_nodes, int32_t root, const uint32_t* d_entries, uint32_t n_entries, float* d_scratch, hipStream_t stream) {
    if (n_entries == 0 || root < 0) return hipErrorInvalidValue;
    const uint32_t nb = sah_blocks(n_entries);
    hipLaunchKernelGGL(sah_terms_kernel, dim3(nb), dim3(IM_BLOCK), 0, stream, d_nodes, d_entries, n_entries, d_scratch + 4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sah_finish_kernel, dim3(1), dim3(IM_BLOCK), 0, stream, d_nodes, root, d_scratch + 4, nb, d_scratch);
    return hipGetLastError();
}

}  // namespace pt
