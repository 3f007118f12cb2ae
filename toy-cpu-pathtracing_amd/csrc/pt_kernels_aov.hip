// The AOV renderers — NormalRenderer::render (renderer/src/renderer/normal_renderer.rs:26-75) and AlbedoRenderer::render
// (renderer/src/renderer/albedo_renderer.rs:30-69) — as a persistent wave64 primary-ray kernel for gfx950, plus the extension
// AOV_SHADING_NORMAL (no reference counterpart: the render-space shading normal of every surface).
//
// Structure: what pt_kernel (pt_kernel.hpp) does for one path vertex, and nothing after it.  One-wave workgroups pull (8x8 tile block,
// sample range) work items from the launch's counter (lane_job), the item's film tile lives in LDS and is written back once.  A work
// item's (pixel, sample) pairs are taken 64 at a time in pool order (sample-major), the tile STARTS from the pixels' sums in the film and
// the sample range of a launch is never split over work items (the host launches with chunks = 1): a pixel's sum is the reference's
// `acc_color += ...` in sample order, continued across calls, so that [0, a) then [a, b) leaves the bits of [0, b).  Every lane draws its
// sample's dimensions with the path kernels' sampler code (block-uniform Sobol prefix tables where the launch shape allows), shoots the
// camera ray of regen_path WITHOUT the path renderers' epsilon (the reference's AOV renderers do not move the ray forward), and the wave
// walks the 64 primary rays with trace_closest_coop.  Primary rays are coherent and every lane is done after one vertex: there is no tail
// queue, no deferral record and no merged traversal here.
//
// Semantics are the reference's, quirks included:
//  * normal: only get_2d_pixel() is drawn (Sobol dimensions 0-1, no wavelength draw in front).  A hit on a BSDF material stores the shading
//    normal AFTER `interaction.shading_transform() * interaction` (samples.rs:130-148; Transform * Normal = inverse-transpose, then
//    normalised, math/src/transform.rs:44-52): the normal in its own tangent frame, (0, 0, 1) up to rounding, so every BSDF surface is
//    (0.5, 0.5, 1.0).  A hit on an emitter stores the render-space shading normal.  Both * 0.5 + 0.5; a miss is 0.  The normal map is not applied;
//  * albedo: get_1d() -> SampledWavelengths::new_uniform, then get_2d_pixel() (the path renderers' first three dimensions);
//    sample_albedo_spectrum(uv, lambda) of the BSDF material (scene/src/material/impls/*.rs) times presets::cie_illum_d6500() at the four
//    wavelengths into Sensor::add_sample with exposure 1.  Emitters and misses add nothing;
//  * shading_normal: the reference's emitter branch of `normal` for every hit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_albedo.hpp"
#include "pt_kernel.hpp"

namespace pt {

enum : uint32_t { AOV_NORMAL = 0, AOV_ALBEDO = 1, AOV_SHADING_NORMAL = 2 };   // = MI355PT_AOV_* (include/mi355pt.h)

// (sample_albedo_spectrum: albedo_spectrum<FEAT> in pt_albedo.hpp, shared with the G-buffer kernel)

template <uint32_t KIND, uint32_t FEAT>
__global__ __launch_bounds__(64, PT_MIN_WAVES) void aov_kernel(DevScene sc, DevCamera cam, DevParams prm, uint32_t illuminant_lut,
                                                               const uint64_t* __restrict__ dim_hash_tab, float* __restrict__ accum,
                                                               unsigned* __restrict__ work_counter, DevStats* __restrict__ stats) {
    constexpr uint32_t N_DIMS = KIND == AOV_ALBEDO ? 2u : 1u;   // draws start at dimensions 0 (get_1d) and 1 (get_2d), or at 0 (get_2d) alone
    __shared__ uint32_t s_stack[STACK_DEPTH * 64];
    __shared__ float s_film[64 * 3];                            // the work item's 8x8 film tile
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
    if constexpr (KIND == AOV_ALBEDO && (FEAT & FEAT_TEX) != 0u) s_znodes[lane] = sc.z_nodes[lane];   // rgb2spec_lookup's z search (pt_device.hpp)
    __syncthreads();
    SamplerCtx sctx{prm.sampler, prm.seed, prm.log2_spp, prm.n_base4_digits, cam.width, dim_hash_tab, nullptr, 0u, 0u, nullptr, s_perm};
    StatCounters st{};
    unsigned long long n_samples = 0ull, n_hits = 0ull;        // wave-uniform (ballot counts)

    for (;;) {
        if (lane == 0) s_work = atomicAdd(work_counter, 1u);
        __syncthreads();
        const uint32_t work = s_work;
        __syncthreads();
        if (work >= prm.n_work) break;
        const LaneJob job = lane_job(work, lane, cam, prm);      // this lane's own pixel of the tile (film write-back)
        const LaneJob job0 = lane_job(work, 0u, cam, prm);       // the block origin and the item's wave-uniform sample range
        const uint32_t blk_log2 = prm.block_log2, blk_mask = (1u << blk_log2) - 1u;
        item_sobol_prefixes(sctx, prm, job0, lane, s_hi, s_p6, N_DIMS);
        // the tile continues the film's sums (this lane's own pixel; lanes without one hold 0 and are never added to)
        const size_t film_o = ((size_t)job.py * cam.width + job.px) * 3;
        float f0 = 0.0f, f1 = 0.0f, f2_ = 0.0f;
        if (job.valid) { f0 = accum[film_o]; f1 = accum[film_o + 1]; f2_ = accum[film_o + 2]; }
        s_film[3 * lane] = f0; s_film[3 * lane + 1] = f1; s_film[3 * lane + 2] = f2_;
        __syncthreads();
        const uint32_t n_s = job0.s_end > job0.s_cur ? job0.s_end - job0.s_cur : 0u;
        const uint32_t pool_size = n_s << (2u * blk_log2);
        for (uint32_t pool_next = 0u; pool_next < pool_size; pool_next += 64u) {
            // the next 64 (pixel, sample) pairs of the pool, sample-major: a pixel's samples reach its sum in index order
            const uint32_t idx = pool_next + lane;
            const uint32_t pix = idx & ((1u << (2u * blk_log2)) - 1u);
            const uint32_t px = job0.px + (pix & blk_mask), py = job0.py + (pix >> blk_log2);
            const bool active = idx < pool_size && px < cam.width && py < cam.height;
            f3 rd = mk3(0.0f, 0.0f, 1.0f);
            Wl wl; wl.lam0 = LAMBDA_MIN; wl.term = false;
            if (active) {
                Sampler smp;
                sampler_start(smp, sctx, px, py, job0.s_cur + (idx >> (2u * blk_log2)));
                if constexpr (KIND == AOV_ALBEDO) wl_init(wl, get_1d(smp, sctx));   // albedo_renderer.rs:47-48
                const f2 uv = get_2d(smp, sctx);                                      // get_2d_pixel
                rd = camera_ray_dir(cam, px, py, uv);                                 // camera.sample_ray: the origin stays where it is
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
                const bool bsdf = mat->type != MT_EMISSIVE;                           // as_bsdf_material().is_some()
                if constexpr (KIND == AOV_ALBEDO) {
                    if (bsdf) {
                        Path P{};
                        P.wl = wl;
                        albedo_spectrum<FEAT>(sc, mat, wl, sf.uv, P.L, st);
                        const float* illum = sc.luts + (size_t)illuminant_lut * 470;
                        float lam[4];
                        wl_lams(wl, lam);
#pragma unroll
                        for (int i = 0; i < 4; ++i) P.L[i] = (P.L[i] * 1.0f) * lut_value(illum, lam[i]);   // (sample * rs.weight).multiply_spectrum(D65)
                        float r, g, b;
                        film_rgb(P, sc, prm, r, g, b);                                // Sensor::add_sample, exposure 1 (prm.exposure)
                        atomicAdd(&s_film[3 * pix], r); atomicAdd(&s_film[3 * pix + 1], g); atomicAdd(&s_film[3 * pix + 2], b);
                    }
                } else {
                    f3 n = sf.ns;
                    if (KIND == AOV_NORMAL && bsdf) {
                        // render_to_tangent * interaction: the normal goes through the inverse-transpose of render -> tangent, whose rows are
                        // the columns of the way back (pt_path.hpp shading_frames_numeric: glam's numeric inverses), and is normalised again
                        Frame fr, fw;
                        shading_frames_numeric(sf.ns, sf.tangent, fr, fw);
                        n = normalize(to_local(fw, sf.ns));
                    }
                    // acc_color += color * rs.weight (the box filter's weight is 1)
                    atomicAdd(&s_film[3 * pix], (n.x * 0.5f + 0.5f) * 1.0f);
                    atomicAdd(&s_film[3 * pix + 1], (n.y * 0.5f + 0.5f) * 1.0f);
                    atomicAdd(&s_film[3 * pix + 2], (n.z * 0.5f + 0.5f) * 1.0f);
                }
            }
        }
        __syncthreads();
        if (job.valid) { accum[film_o] = s_film[3 * lane]; accum[film_o + 1] = s_film[3 * lane + 1]; accum[film_o + 2] = s_film[3 * lane + 2]; }
        __syncthreads();
    }
    if (stats != nullptr && lane == 0) {
        atomicAdd(&stats->samples, n_samples);
        atomicAdd(&stats->closest_rays, n_samples);
        atomicAdd(&stats->closest_hits, n_hits);
    }
}

// RendererImage's pixel from the linear sums.  normal / shading_normal: acc / spp, stored raw (ColorSrgb<NoneToneMap>::from_rgb,
// normal_renderer.rs:71-73).  albedo: Sensor::to_rgb with NoneToneMap and the sRGB OETF (sensor.rs:81-88): mean, clip at 0 from below, OETF —
// values above 1 stay.
__global__ void aov_resolve_kernel(uint32_t kind, const float* __restrict__ accum, uint32_t n_values, uint32_t spp, float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (; i < n_values; i += stride) {
        float c = accum[i] / (float)spp;
        if (kind == AOV_ALBEDO) c = srgb_oetf(fmaxf(c, 0.0f));
        out[i] = c;
    }
}

// ---- host side (declared in launch.hpp for api.cpp) ----
// the instantiation a (kind, scene feature set) launches: texture code only in the albedo kernel of a scene with spectrum textures
using AovKernel = void (*)(DevScene, DevCamera, DevParams, uint32_t, const uint64_t*, float*, unsigned*, DevStats*);
static AovKernel find_aov_kernel(uint32_t kind, uint32_t feat) {
    if (kind == AOV_NORMAL) return aov_kernel<AOV_NORMAL, 0u>;
    if (kind == AOV_SHADING_NORMAL) return aov_kernel<AOV_SHADING_NORMAL, 0u>;
    return (feat & FEAT_TEX) != 0u ? aov_kernel<AOV_ALBEDO, FEAT_TEX> : aov_kernel<AOV_ALBEDO, 0u>;
}

hipError_t launch_aov(uint32_t kind, const DevScene& sc, const DevCamera& cam, const DevParams& prm, uint32_t illuminant_lut, const uint64_t* d_hash,
                      float* d_accum, unsigned* d_counter, DevStats* d_stats, uint32_t feat, int grid, hipStream_t stream) {
    if (prm.chunks != 1u) return hipErrorInvalidValue;      // (a pixel's sum is sequential in the sample index: see the top of this file)
    hipLaunchKernelGGL(find_aov_kernel(kind, feat), dim3(grid), dim3(64), 0, stream, sc, cam, prm, illuminant_lut, d_hash, d_accum, d_counter, d_stats);
    return hipGetLastError();
}
// resident 64-thread blocks (= waves) of that instantiation on the current device: the persistent grid size
int query_resident_waves_aov(uint32_t kind, uint32_t feat) { return resident_waves_of(find_aov_kernel(kind, feat)); }
hipError_t launch_aov_resolve(uint32_t kind, const float* d_accum, uint32_t n_values, uint32_t spp, float* d_out, hipStream_t stream) {
    if (n_values == 0u) return hipSuccess;
    int grid = (int)std::min<uint32_t>((n_values + 255) / 256, 2048u);
    hipLaunchKernelGGL(aov_resolve_kernel, dim3(grid), dim3(256), 0, stream, kind, d_accum, n_values, spp, d_out);
    return hipGetLastError();
}

}  // namespace pt
