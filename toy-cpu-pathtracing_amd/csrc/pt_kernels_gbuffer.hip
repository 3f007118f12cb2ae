// The G-buffer pass (include/mi355pt_gbuffer.h): ONE primary-ray launch that writes up to four films — albedo, shading normal, hit
// position, hit record — from the same rays.  EXTENSION, no reference counterpart as a renderer; the albedo film is the reference's
// AlbedoRenderer sample for sample (pt_kernels_aov.hip's AOV_ALBEDO, bit for bit).
//
// Structure: aov_kernel's (pt_kernels_aov.hip).  One-wave workgroups pull (8x8 tile, sample range) work items from the launch's counter; the
// host plans the launch with block_log2 = 3 and chunks = 1 ALWAYS, so lane l owns pixel (l & 7, l >> 3) of the tile for the whole item and
// the item's samples reach the pixel in index order.  That is why there is no film tile in LDS here: a pixel's twelve sums (four films x
// three channels) live in the owning lane's registers, start from the values in the films, take one plain f32 add per sample and are
// stored once — no atomics, and the LDS footprint is the AOV kernel's minus its tile.  [0, a) then [a, b) leaves the bits of [0, b).
//
// Per (pixel, sample index) the schedule is the albedo renderer's WHICHEVER films are requested: get_1d() (wavelengths), get_2d_pixel(),
// camera_ray_dir from the origin without RAY_EPS, trace_closest_coop, load_surface once.  A film is requested when its pointer is non-NULL;
// the choice is a launch constant, so a runtime (wave-uniform) branch serves and a film never depends on which other films were asked for.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_albedo.hpp"
#include "pt_kernel.hpp"

namespace pt {

template <uint32_t FEAT>
__global__ __launch_bounds__(64, PT_MIN_WAVES) void gbuffer_kernel(DevScene sc, DevCamera cam, DevParams prm, uint32_t illuminant_lut,
                                                                   const uint64_t* __restrict__ dim_hash_tab, GbufferFilms films,
                                                                   unsigned* __restrict__ work_counter, DevStats* __restrict__ stats) {
    constexpr uint32_t N_DIMS = 2u;                              // dimensions 0 (get_1d) and 1 (get_2d)
    __shared__ uint32_t s_stack[STACK_DEPTH * 64];
    __shared__ uint32_t s_hi[N_DIMS];
    __shared__ uint32_t s_p6[N_DIMS];
    __shared__ unsigned s_work;
    __shared__ uint8_t s_perm[96];
    __shared__ uint32_t s_ring[ANY_RING];
    __shared__ uint32_t s_pair[64];
    __shared__ unsigned long long s_best[64];
    const ClosestLds closest_lds{s_ring, s_best, s_pair};
    const uint32_t lane = threadIdx.x;
    uint32_t* stack = s_stack + lane;
    for (uint32_t k = lane; k < 96u; k += 64u) s_perm[k] = (uint8_t)((perm_packed(k >> 2) >> (2u * (k & 3u))) & 3u);
    if constexpr ((FEAT & FEAT_TEX) != 0u) s_znodes[lane] = sc.z_nodes[lane];   // rgb2spec_lookup's z search (pt_device.hpp)
    __syncthreads();
    SamplerCtx sctx{prm.sampler, prm.seed, prm.log2_spp, prm.n_base4_digits, cam.width, dim_hash_tab, nullptr, 0u, 0u, nullptr, s_perm};
    StatCounters st{};
    unsigned long long n_samples = 0ull, n_hits = 0ull;        // wave-uniform (ballot counts)
    const bool want_a = films.albedo != nullptr, want_n = films.shading_normal != nullptr, want_p = films.position != nullptr,
               want_h = films.hit != nullptr;                   // launch constants

    for (;;) {
        if (lane == 0) s_work = atomicAdd(work_counter, 1u);
        __syncthreads();
        const uint32_t work = s_work;
        __syncthreads();
        if (work >= prm.n_work) break;
        const LaneJob job = lane_job(work, lane, cam, prm);      // block_log2 == 3: this lane's own pixel of the 8x8 tile
        const LaneJob job0 = lane_job(work, 0u, cam, prm);       // the tile origin and the item's wave-uniform sample range
        item_sobol_prefixes(sctx, prm, job0, lane, s_hi, s_p6, N_DIMS);
        // the sums continue the films' (lanes without a pixel hold 0, are never added to and never stored)
        const size_t film_o = ((size_t)job.py * cam.width + job.px) * 3;
        f3 acc_a = mk3(0.0f, 0.0f, 0.0f), acc_n = acc_a, acc_p = acc_a, acc_h = acc_a;
        if (job.valid) {
            if (want_a) acc_a = mk3(films.albedo[film_o], films.albedo[film_o + 1], films.albedo[film_o + 2]);
            if (want_n) acc_n = mk3(films.shading_normal[film_o], films.shading_normal[film_o + 1], films.shading_normal[film_o + 2]);
            if (want_p) acc_p = mk3(films.position[film_o], films.position[film_o + 1], films.position[film_o + 2]);
            if (want_h) acc_h = mk3(films.hit[film_o], films.hit[film_o + 1], films.hit[film_o + 2]);
        }
        __syncthreads();                                         // the prefix tables are written
        for (uint32_t s = job0.s_cur; s < job0.s_end; ++s) {
            const bool active = job.valid;
            f3 rd = mk3(0.0f, 0.0f, 1.0f);
            Wl wl; wl.lam0 = LAMBDA_MIN; wl.term = false;
            if (active) {
                Sampler smp;
                sampler_start(smp, sctx, job.px, job.py, s);
                wl_init(wl, get_1d(smp, sctx));                  // albedo_renderer.rs:47-48 — drawn whether or not the albedo film is wanted
                const f2 uv = get_2d(smp, sctx);                 // get_2d_pixel
                rd = camera_ray_dir(cam, job.px, job.py, uv);    // camera.sample_ray: the origin stays where it is
            }
            Hit hit{};
            PT_PRIO_TRAV_ENTER;
            const bool got = trace_closest_coop<false>(sc, mk3(0.0f, 0.0f, 0.0f), rd, active, stack, lane, closest_lds, hit, st);
            PT_PRIO_TRAV_EXIT;
            n_samples += (unsigned long long)__popcll(__ballot(active));
            n_hits += (unsigned long long)__popcll(__ballot(got));
            if (got) {
                const Surface sf = load_surface(sc, hit, rd);
                const DevMaterial* mat = sc.materials + sf.material;
                const bool bsdf = mat->type != MT_EMISSIVE;      // as_bsdf_material().is_some()
                if (want_a && bsdf) {                            // aov_kernel<AOV_ALBEDO, FEAT>'s statements
                    Path P{};
                    P.wl = wl;
                    albedo_spectrum<FEAT>(sc, mat, wl, sf.uv, P.L, st);
                    const float* illum = sc.luts + (size_t)illuminant_lut * 470;
                    float lam[4];
                    wl_lams(wl, lam);
#pragma unroll
                    for (int i = 0; i < 4; ++i) P.L[i] = (P.L[i] * 1.0f) * lut_value(illum, lam[i]);   // (sample * rs.weight).multiply_spectrum(D65)
                    float r, g, b;
                    film_rgb(P, sc, prm, r, g, b);               // Sensor::add_sample, exposure 1 (prm.exposure)
                    acc_a.x += r; acc_a.y += g; acc_a.z += b;
                }
                if (want_n) {                                    // AOV_SHADING_NORMAL's expression, emitters included
                    acc_n.x += (sf.ns.x * 0.5f + 0.5f) * 1.0f;
                    acc_n.y += (sf.ns.y * 0.5f + 0.5f) * 1.0f;
                    acc_n.z += (sf.ns.z * 0.5f + 0.5f) * 1.0f;
                }
                if (want_p) { acc_p.x += sf.p.x; acc_p.y += sf.p.y; acc_p.z += sf.p.z; }   // render space: the camera is the origin
                if (want_h) { acc_h.x += hit.t; acc_h.y += 1.0f; acc_h.z += bsdf ? 0.0f : 1.0f; }
            }
        }
        if (job.valid) {
            if (want_a) { films.albedo[film_o] = acc_a.x; films.albedo[film_o + 1] = acc_a.y; films.albedo[film_o + 2] = acc_a.z; }
            if (want_n) { films.shading_normal[film_o] = acc_n.x; films.shading_normal[film_o + 1] = acc_n.y; films.shading_normal[film_o + 2] = acc_n.z; }
            if (want_p) { films.position[film_o] = acc_p.x; films.position[film_o + 1] = acc_p.y; films.position[film_o + 2] = acc_p.z; }
            if (want_h) { films.hit[film_o] = acc_h.x; films.hit[film_o + 1] = acc_h.y; films.hit[film_o + 2] = acc_h.z; }
        }
        __syncthreads();                                         // the next item rewrites the prefix tables
    }
    if (stats != nullptr && lane == 0) {
        atomicAdd(&stats->samples, n_samples);
        atomicAdd(&stats->closest_rays, n_samples);
        atomicAdd(&stats->closest_hits, n_hits);
    }
}

// Coverage-normalised means: out = film / hit.y per value where the pixel's hit count is > 0, else 0 (film may be the hit film itself:
// .x becomes the mean distance, .y 1, .z the emitter share of the hits).
__global__ void gbuffer_normalize_kernel(const float* __restrict__ film, const float* __restrict__ hit, uint32_t n_pixels, float* __restrict__ out) {
    const size_t n_values = (size_t)n_pixels * 3u;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_values; i += stride) {
        const float cnt = hit[(i / 3u) * 3u + 1u];
        out[i] = cnt > 0.0f ? film[i] / cnt : 0.0f;
    }
}

// ---- host side (declared in launch.hpp for api.cpp) ----
using GbufferKernel = void (*)(DevScene, DevCamera, DevParams, uint32_t, const uint64_t*, GbufferFilms, unsigned*, DevStats*);
static GbufferKernel find_gbuffer_kernel(uint32_t feat) { return (feat & FEAT_TEX) != 0u ? gbuffer_kernel<FEAT_TEX> : gbuffer_kernel<0u>; }

hipError_t launch_gbuffer(const DevScene& sc, const DevCamera& cam, const DevParams& prm, uint32_t illuminant_lut, const uint64_t* d_hash,
                          const GbufferFilms& films, unsigned* d_counter, DevStats* d_stats, uint32_t feat, int grid, hipStream_t stream) {
    // one pixel per lane and sums that are sequential in the sample index: see the top of this file
    if (prm.chunks != 1u || prm.block_log2 != 3u || prm.sample_prefix_digits != 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(find_gbuffer_kernel(feat), dim3(grid), dim3(64), 0, stream, sc, cam, prm, illuminant_lut, d_hash, films, d_counter, d_stats);
    return hipGetLastError();
}
int query_resident_waves_gbuffer(uint32_t feat) { return resident_waves_of(find_gbuffer_kernel(feat)); }
hipError_t launch_gbuffer_normalize(const float* d_film, const float* d_hit, uint32_t n_pixels, float* d_out, hipStream_t stream) {
    if (n_pixels == 0u) return hipSuccess;
    const int grid = (int)std::min<size_t>(((size_t)n_pixels * 3u + 255u) / 256u, (size_t)2048);
    hipLaunchKernelGGL(gbuffer_normalize_kernel, dim3(grid), dim3(256), 0, stream, d_film, d_hit, n_pixels, d_out);
    return hipGetLastError();
}

}  // namespace pt
