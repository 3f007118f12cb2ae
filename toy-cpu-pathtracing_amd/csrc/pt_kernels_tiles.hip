// Path renders over an explicit tile list: the generic-mode instantiations of pt_kernel_tiles (pt_kernel_tiles.hpp; strategy and sampler
// read from DevParams, like pt_kernels.hip's) and the combine kernel for lists (launched by pt_kernels.hip's launch_pt).
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

}  // namespace pt

PT_KERNELS_TILES_CC(MODE_GENERIC)
PT_KERNELS_TILES_PLAIN(MODE_GENERIC)
