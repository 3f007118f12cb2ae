// Adaptive sampling's noise step (include/mi355pt_adaptive.h, which is normative for the arithmetic and its order): streaming wave64
// kernels for gfx950 over the film F, the half film H and the per-tile counts.
//   adaptive_err_kernel      one wave per 8x8 tile (lane = pixel (lane & 7, lane >> 3) of the tile: a row of the tile is 96 contiguous
//                            bytes of each film), four tiles per 256-thread block, grid-stride over the tiles.  Tiles whose count is not
//                            level_spp are skipped after ONE dword.  The 64 per-pixel errors are summed by a xor butterfly over
//                            32, 16, .. 1 lanes: binary32 addition is commutative, so every lane holds the sum of the header's pairwise tree and
//                            the decision is wave-uniform.  An active tile copies H := F from the registers that hold F and doubles its count.
//   adaptive_compact_kernel  ONE block of 16 waves turns the per-tile flags into the ascending list: 1 024 tiles per round, a ballot and a
//                            popcount per wave, the waves' counts through LDS.  32 rounds at 1920 x 1080 (32 400 tiles).
//   normalize_tiles_kernel   F / (float)tile_spp per value, one thread per pixel.
// No float atomics, no dependence on the schedule: two runs are bit-equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "launch.hpp"

namespace pt {

namespace {

constexpr uint32_t AD_BLOCK = 256, AD_TILES_PER_BLOCK = AD_BLOCK / 64, AD_COMPACT_BLOCK = 1024, AD_COMPACT_WAVES = AD_COMPACT_BLOCK / 64;

__global__ __launch_bounds__(AD_BLOCK) void adaptive_err_kernel(const float* __restrict__ film, float* __restrict__ half, uint32_t width, uint32_t height,
                                                                uint32_t tiles_x, uint32_t n_tiles, uint32_t* __restrict__ tile_spp,
                                                                float* __restrict__ tile_err, uint32_t* __restrict__ flags, float threshold,
                                                                float dark_eps, uint32_t level_spp, uint32_t max_spp) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float n_full = (float)level_spp, n_half = (float)(level_spp / 2u);
    for (uint32_t tile = blockIdx.x * AD_TILES_PER_BLOCK + wave; tile < n_tiles; tile += gridDim.x * AD_TILES_PER_BLOCK) {
        if (tile_spp[tile] != level_spp) { if (lane == 0) flags[tile] = 0u; continue; }      // wave-uniform
        const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
        const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
        const bool in = px < width && py < height;
        const size_t o = ((size_t)py * width + px) * 3u;
        float fr = 0.0f, fg = 0.0f, fb = 0.0f, e = 0.0f;
        if (in) {
            fr = film[o]; fg = film[o + 1]; fb = film[o + 2];
            const float mr = fr / n_full, mg = fg / n_full, mb = fb / n_full;
            const float hr = half[o] / n_half, hg = half[o + 1] / n_half, hb = half[o + 2] / n_half;
            const float d = (fabsf(mr - hr) + fabsf(mg - hg)) + fabsf(mb - hb);
            const float s = fmaxf((mr + mg) + mb, 0.0f) + dark_eps;
            e = d / sqrtf(s);
        }
        const uint32_t count = (uint32_t)__popcll(__ballot(in));           // >= 1: a tile of the frame has its first pixel inside
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) e = e + __shfl_xor(e, d);
        const float e_t = __shfl(e, 0) / (float)count;
        const bool active = !(e_t <= threshold) && level_spp < max_spp;
        if (lane == 0) { tile_err[tile] = e_t; flags[tile] = active ? 1u : 0u; if (active) tile_spp[tile] = 2u * level_spp; }
        if (active && in) { half[o] = fr; half[o + 1] = fg; half[o + 2] = fb; }
    }
}

__global__ __launch_bounds__(AD_COMPACT_BLOCK) void adaptive_compact_kernel(const uint32_t* __restrict__ flags, uint32_t n_tiles, uint32_t* __restrict__ list,
                                                                            uint32_t* __restrict__ count) {
    __shared__ uint32_t s_cnt[AD_COMPACT_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0u;
    for (uint32_t t0 = 0u; t0 < n_tiles; t0 += AD_COMPACT_BLOCK) {          // (n_tiles < 2^31: launch_adaptive_step)
        const uint32_t t = t0 + threadIdx.x;
        const bool a = t < n_tiles && flags[t] != 0u;
        const unsigned long long m = __ballot(a);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < AD_COMPACT_WAVES; ++w) { const uint32_t c = s_cnt[w]; before += w < wave ? c : 0u; total += c; }
        if (a) list[base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t;    // at most n_tiles entries: the list's size
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

__global__ __launch_bounds__(256) void normalize_tiles_kernel(const float* film, const uint32_t* __restrict__ tile_spp, uint32_t width,
                                                              uint32_t height, uint32_t tiles_x, float* mean) {     // (mean may be film)
    const size_t n_pix = (size_t)width * height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t px = (uint32_t)(i % width), py = (uint32_t)(i / width);
        const float n = (float)tile_spp[(py >> 3) * tiles_x + (px >> 3)];
        mean[3 * i] = film[3 * i] / n; mean[3 * i + 1] = film[3 * i + 1] / n; mean[3 * i + 2] = film[3 * i + 2] / n;
    }
}

}  // namespace

// tiles of a width x height frame, 0 when the frame is empty or has 2^31 tiles or more
uint32_t adaptive_tile_count(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)((width + 7ull) / 8ull) * ((height + 7ull) / 8ull);
    return n < (1ull << 31) ? (uint32_t)n : 0u;
}
// one u32 flag per tile, rounded up to 16 bytes, and 16 bytes at the end for the drivers' count (api.cpp); 0 for a frame without tiles
size_t adaptive_scratch_bytes(uint32_t width, uint32_t height) {
    const size_t n = adaptive_tile_count(width, height);
    return n ? ((n * 4u + 15u) & ~(size_t)15u) + 16u : 0u;
}

hipError_t launch_adaptive_step(const float* d_film, float* d_half, uint32_t width, uint32_t height, uint32_t* d_tile_spp, float* d_tile_err,
                                float threshold, float dark_eps, uint32_t level_spp, uint32_t max_spp, void* d_scratch, uint32_t* d_list,
                                uint32_t* d_count, hipStream_t stream) {
    const uint32_t n_tiles = adaptive_tile_count(width, height), tiles_x = (width + 7u) / 8u;
    if (n_tiles == 0u) return hipErrorInvalidValue;
    const uint32_t grid = std::min<uint32_t>((n_tiles + AD_TILES_PER_BLOCK - 1u) / AD_TILES_PER_BLOCK, 2048u);
    hipLaunchKernelGGL(adaptive_err_kernel, dim3(grid), dim3(AD_BLOCK), 0, stream, d_film, d_half, width, height, tiles_x, n_tiles, d_tile_spp, d_tile_err,
                       (uint32_t*)d_scratch, threshold, dark_eps, level_spp, max_spp);
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(AD_COMPACT_BLOCK), 0, stream, (const uint32_t*)d_scratch, n_tiles, d_list, d_count);
    return hipGetLastError();
}

hipError_t launch_adaptive_compact(const uint32_t* d_flags, uint32_t n_tiles, uint32_t* d_list, uint32_t* d_count, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(AD_COMPACT_BLOCK), 0, stream, d_flags, n_tiles, d_list, d_count);
    return hipGetLastError();
}

hipError_t launch_normalize_tiles(const float* d_film, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_mean, hipStream_t stream) {
    if (adaptive_tile_count(width, height) == 0u) return hipErrorInvalidValue;
    const size_t n_pix = (size_t)width * height;
    const uint32_t grid = (uint32_t)std::min<size_t>((n_pix + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(normalize_tiles_kernel, dim3(grid), dim3(256), 0, stream, d_film, d_tile_spp, width, height, (width + 7u) / 8u, d_mean);
    return hipGetLastError();
}

}  // namespace pt
