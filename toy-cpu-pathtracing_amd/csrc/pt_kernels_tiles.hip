// Path renders over an explicit tile list: the generic-mode instantiations of pt_kernel_tiles (pt_kernel_tiles.hpp; strategy and sampler
// read from DevParams, like pt_kernels.hip's), the combine kernel for lists and the launcher api.cpp calls (launch.hpp).
#include <hip/hip_runtime.h>

#include "pt_kernel_tiles.hpp"

namespace pt {

// combine_kernel (pt_kernels.hip) for a list: adds the per-chunk film tiles of a split launch to the film, in chunk order (one thread per
// pixel of each listed tile; slots are laid out by position in the list).  An index beyond the frame selects no pixel, as in lane_job_tiles.
__global__ void combine_tiles_kernel(DevCamera cam, DevParams prm, const float* __restrict__ partial, float* __restrict__ accum, uint32_t n_list) {
    const uint32_t tile_k = blockIdx.x, lane = threadIdx.x;
    if (tile_k >= n_list) return;
    const uint32_t tile = min(tile_list(prm)[tile_k], prm.tiles_x * prm.tiles_y);
    const uint32_t px = (tile % prm.tiles_x) * 8u + (lane & 7u), py = (tile / prm.tiles_x) * 8u + (lane >> 3);
    if (px >= cam.width || py >= cam.height) return;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (uint32_t c = 0; c < prm.chunks; ++c) {
        const float* slot = partial + (((size_t)tile_k * prm.chunks + c) * 64u + lane) * 3u;
        r += slot[0]; g += slot[1]; b += slot[2];
    }
    const size_t o = ((size_t)py * cam.width + px) * 3;
    accum[o] += r; accum[o + 1] += g; accum[o + 2] += b;
}

hipError_t launch_pt_tiles(const DevScene& sc, const DevCamera& cam, const DevParams& prm, uint32_t n_list, const uint64_t* d_hash, float* d_accum,
                           float* d_partial, unsigned* d_counter, uint32_t feat, int grid, hipStream_t stream, float* d_defer) {
    const PtLaunchArgs a{sc, cam, prm, d_hash, d_accum, d_partial, d_counter, nullptr, grid, stream, PathOut{nullptr, nullptr, nullptr, 0u, 0u}, (float4*)d_defer};
    // the MODE of launch_pt (pt_kernels.hip) for the same strategy and sampler
    if (prm.sampler == 1u && prm.strategy == 2u) launch_pt_tiles_mis_sobol(a, feat);
    else if (prm.sampler == 1u && prm.strategy == 1u) launch_pt_tiles_nee_sobol(a, feat);
    else if (prm.strategy == 0u) launch_pt_tiles_strategy_pt(a, feat);
    else if (pick_features(feat) & FEAT_CC) launch_pt_tiles_cc<MODE_GENERIC>(a, feat);
    else launch_pt_tiles_plain<MODE_GENERIC>(a, feat);
    if (prm.chunks > 1)
        hipLaunchKernelGGL(combine_tiles_kernel, dim3(n_list), dim3(64), 0, stream, cam, prm, (const float*)d_partial, d_accum, n_list);
    return hipGetLastError();
}

}  // namespace pt
