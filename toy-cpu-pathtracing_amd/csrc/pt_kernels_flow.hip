// The flow pass (include/mi355pt_flow.h): where the point a pixel shows was one frame ago — ONE primary ray through every pixel CENTRE, and
// from the closest hit's triangle and barycentrics the displacement of that point and the change of the facet normal between the scene's
// mark (the render-space positions of the previous frame, mi355pt_scene_flow_mark) and the current positions, as one 32-byte record per
// pixel, with the ID pass's instance + 1.  EXTENSION, no reference counterpart.  The flow-aware temporal accumulation adds a pixel's record.
//
// Structure: ids_kernel's (pt_kernels_ids.hip).  One-wave workgroups pull 8x8 tiles from the launch's counter; the host plans the launch
// with block_log2 = 3 and chunks = 1, so lane l owns pixel (l & 7, l >> 3) of the tile.  One trace_closest_coop<false> per item.  Both
// 48-byte triangle records are then loaded as three 16-byte loads each, UNCONDITIONALLY — of the hit's triangle, or of triangle 0 for a
// lane without a hit (the host refuses a scene without triangles) —, all six in flight together; the record leaves as two 16-byte stores.
// No sampler, no film tile, no LDS but the traversal's, no atomics but the work counter and the statistics, no material.
//
// Every operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls no
// fmaf); division and sqrtf are IEEE (hipcc's default: correctly rounded): the records are bit-equal to tests/flow_reference.py.
//
// DEBUG: the same kernel also writes {tri, b0, b1, b2} of the hit per pixel (mi355pt_render_flow_debug, include/mi355pt_debug.h).
#include <hip/hip_runtime.h>

#include "pt_kernel.hpp"

namespace pt {

namespace {

// the facet normal of the header: cross(P1 - P0, P2 - P0) / sqrtf(dot); `ok`: the squared length is finite and not 0
PT_DEV f3 flow_facet_normal(f3 p0, f3 p1, f3 p2, bool& ok) {
    const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
    const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const float l2 = (cx * cx + cy * cy) + cz * cz;
    ok = l2 > 0.0f && l2 <= 3.402823466e+38f;
    const float l = sqrtf(l2);
    return mk3(cx / l, cy / l, cz / l);
}

template <bool DEBUG>
__global__ __launch_bounds__(64, PT_MIN_WAVES) void flow_kernel(DevScene sc, DevCamera cam, DevParams prm, const DevTri* __restrict__ tris_prev,
                                                                float4* __restrict__ flow, uint32_t* __restrict__ ids, float4* __restrict__ hits,
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

        // the two records of the hit's triangle (of triangle 0 without a hit: loaded, selected away below)
        const uint32_t tri = got ? hit.tri : 0u;
        const float4* const qc = (const float4*)(sc.tris_render + tri);
        const float4* const qv = (const float4*)(tris_prev + tri);
        const float4 ca = qc[0], cb = qc[1], cc = qc[2], va = qv[0], vb = qv[1], vc = qv[2];      // p0 p1x | p1yz p2xy | p2z instance flags mclass
        const f3 c0 = mk3(ca.x, ca.y, ca.z), c1 = mk3(ca.w, cb.x, cb.y), c2 = mk3(cb.z, cb.w, cc.x);
        const f3 v0 = mk3(va.x, va.y, va.z), v1 = mk3(va.w, vb.x, vb.y), v2 = mk3(vb.z, vb.w, vc.x);
        const float b0 = hit.b0, b1 = hit.b1, b2 = hit.b2;
        const float xcx = (b0 * c0.x + b1 * c1.x) + b2 * c2.x, xcy = (b0 * c0.y + b1 * c1.y) + b2 * c2.y, xcz = (b0 * c0.z + b1 * c1.z) + b2 * c2.z;
        const float xvx = (b0 * v0.x + b1 * v1.x) + b2 * v2.x, xvy = (b0 * v0.y + b1 * v1.y) + b2 * v2.y, xvz = (b0 * v0.z + b1 * v1.z) + b2 * v2.z;
        bool okc, okv;
        const f3 nc = flow_facet_normal(c0, c1, c2, okc), nv = flow_facet_normal(v0, v1, v2, okv);
        const bool okn = okc && okv;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t id = 0u;
        if (got) {
            id = __float_as_uint(cc.y) + 1u;                     // DevTri::instance: the render record carries the local record's (ids_kernel reads that one)
            r0 = make_float4(xvx - xcx, xvy - xcy, xvz - xcz, __uint_as_float(id));
            r1 = make_float4(okn ? nv.x - nc.x : 0.0f, okn ? nv.y - nc.y : 0.0f, okn ? nv.z - nc.z : 0.0f, 0.0f);
        }
        if (active) {                                            // job.valid: px < width, py < height
            const size_t p = (size_t)job.py * cam.width + job.px;
            flow[2 * p] = r0;
            flow[2 * p + 1] = r1;
            if (ids != nullptr) ids[p] = id;
            if constexpr (DEBUG) hits[p] = got ? make_float4(__uint_as_float(hit.tri), b0, b1, b2) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    if (stats != nullptr && lane == 0) {
        atomicAdd(&stats->samples, n_rays);
        atomicAdd(&stats->closest_rays, n_rays);
        atomicAdd(&stats->closest_hits, n_hits);
    }
}

}  // namespace

// ---- host side (declared in launch.hpp for api_flow.cpp and api_debug.cpp) ----
hipError_t launch_flow(const DevScene& sc, const DevCamera& cam, const DevParams& prm, const DevTri* d_tris_prev, FlowPixelDev* d_flow, uint32_t* d_ids,
                       void* d_hits, unsigned* d_counter, DevStats* d_stats, int grid, hipStream_t stream) {
    if (prm.chunks != 1u || prm.block_log2 != 3u) return hipErrorInvalidValue;     // one pixel per lane: see the top of this file
    if (sc.n_tris == 0u || d_tris_prev == nullptr || d_flow == nullptr) return hipErrorInvalidValue;      // the unconditional loads read triangle 0
    if (d_hits) hipLaunchKernelGGL(flow_kernel<true>, dim3(grid), dim3(64), 0, stream, sc, cam, prm, d_tris_prev, (float4*)d_flow, d_ids, (float4*)d_hits, d_counter, d_stats);
    else hipLaunchKernelGGL(flow_kernel<false>, dim3(grid), dim3(64), 0, stream, sc, cam, prm, d_tris_prev, (float4*)d_flow, d_ids, (float4*)nullptr, d_counter, d_stats);
    return hipGetLastError();
}
int query_resident_waves_flow(bool debug) { return debug ? resident_waves_of(flow_kernel<true>) : resident_waves_of(flow_kernel<false>); }

}  // namespace pt
