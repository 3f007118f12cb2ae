// The ID pass (include/mi355pt_motion.h): which instance a pixel shows — ONE primary ray through every pixel CENTRE, the closest hit's
// DevTri::instance + 1 (0 for a miss) as one u32 per pixel.  EXTENSION, no reference counterpart.  The motion-aware temporal accumulation
// looks a pixel's motion record up by it.
//
// Structure: gbuffer_kernel's (pt_kernels_gbuffer.hip).  One-wave workgroups pull 8x8 tiles from the launch's counter; the host plans the
// launch with block_log2 = 3 and chunks = 1, so lane l owns pixel (l & 7, l >> 3) of the tile.  One trace_closest_coop<false> per item, one
// u32 store per lane that has a pixel.  No sampler (uv = (0.5, 0.5): spp, seed and sampler do not matter), so none of its tables; no film
// tile; no atomics but the work counter and the statistics; no material is touched, so there is no FEAT template.
#include <hip/hip_runtime.h>

#include "pt_kernel.hpp"

namespace pt {

__global__ __launch_bounds__(64, PT_MIN_WAVES) void ids_kernel(DevScene sc, DevCamera cam, DevParams prm, uint32_t* __restrict__ ids,
                                                               unsigned* __restrict__ work_counter, DevStats* __restrict__ stats) {
    __shared__ uint32_t s_stack[STACK_DEPTH * 64];
    __shared__ unsigned s_work;
    __shared__ uint32_t s_ring[ANY_RING];
    __shared__ uint32_t s_pair[64];
    __shared__ unsigned long long s_best[64];
    const ClosestLds closest_lds{s_ring, s_best, s_pair};
    const uint32_t lane = threadIdx.x;
    uint32_t* stack = s_stack + lane;
    StatCounters st{};
    unsigned long long n_rays = 0ull, n_hits = 0ull;            // wave-uniform (ballot counts)

    for (;;) {
        if (lane == 0) s_work = atomicAdd(work_counter, 1u);
        __syncthreads();
        const uint32_t work = s_work;
        __syncthreads();
        if (work >= prm.n_work) break;
        const LaneJob job = lane_job(work, lane, cam, prm);      // block_log2 == 3: this lane's own pixel of the 8x8 tile
        const bool active = job.valid;
        f3 rd = mk3(0.0f, 0.0f, 1.0f);
        if (active) rd = camera_ray_dir(cam, job.px, job.py, f2{0.5f, 0.5f});   // camera.sample_ray at the pixel centre: the origin stays where it is
        Hit hit{};
        PT_PRIO_TRAV_ENTER;
        const bool got = trace_closest_coop<false>(sc, mk3(0.0f, 0.0f, 0.0f), rd, active, stack, lane, closest_lds, hit, st);
        PT_PRIO_TRAV_EXIT;
        n_rays += (unsigned long long)__popcll(__ballot(active));
        n_hits += (unsigned long long)__popcll(__ballot(got));
        uint32_t id = 0u;
        if (got) id = ((const uint32_t*)(sc.tris_local + hit.tri))[9] + 1u;      // DevTri::instance (load_tri_local's word)
        if (active) ids[(size_t)job.py * cam.width + job.px] = id;               // job.valid: px < width, py < height
    }
    if (stats != nullptr && lane == 0) {
        atomicAdd(&stats->samples, n_rays);
        atomicAdd(&stats->closest_rays, n_rays);
        atomicAdd(&stats->closest_hits, n_hits);
    }
}

// ---- host side (declared in launch.hpp for api_motion.cpp) ----
hipError_t launch_ids(const DevScene& sc, const DevCamera& cam, const DevParams& prm, uint32_t* d_ids, unsigned* d_counter, DevStats* d_stats, int grid,
                      hipStream_t stream) {
    if (prm.chunks != 1u || prm.block_log2 != 3u) return hipErrorInvalidValue;     // one pixel per lane: see the top of this file
    hipLaunchKernelGGL(ids_kernel, dim3(grid), dim3(64), 0, stream, sc, cam, prm, d_ids, d_counter, d_stats);
    return hipGetLastError();
}
int query_resident_waves_ids() { return resident_waves_of(ids_kernel); }

}  // namespace pt
