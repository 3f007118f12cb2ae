// The sample loop of BaseSrgbRenderer::render (renderer/src/renderer/base_renderer.rs:146-280) as a
// persistent wave64 kernel for gfx950.
//
// Structure (MI355X-first, not the reference's depth-first per-pixel recursion):
//  * one wave owns an 8x8 pixel tile x sample range at a time; its paths form a pool of (pixel, sample) pairs handed out
//    sample-major to whichever lane needs a new path, so no lane idles while another still has samples of "its" pixel left
//    (lanes busy at shading 89 % -> 97 % at 64 samples per item, 71 % -> 81 % at 8).  The tile's film is 768 B of LDS updated
//    with ds_add_f32 and written back once per work item; the hand-out order is a function of the wave's own lock-step
//    schedule, so frames are bit-identical from run to run (when the sample range of a tile is split over several work items,
//    each writes its own slot and combine_kernel adds the slots in chunk order: no float atomics on the film);
//  * waves are persistent: they pull (tile, sample-chunk) work items from a global counter;
//  * path state never round-trips through HBM: every lane carries its path in registers and
//    regenerates the next sample of its pixel when the path ends (in-register compaction);
//  * inside a wave the path loop is a lock-step state machine: every iteration all 64 lanes regenerate (those without a path),
//    trace together — ONE cooperative traversal for the closest-hit rays and the pending light connections —, run the FRONT
//    of their vertex together (emission, throughput, Russian roulette); a path that goes on is written to the wave's own queue
//    in global memory (80 B) and frees its lane, and whenever 64 paths wait one pass runs the rest of the vertex — surface,
//    frames, BSDF sample, light connection — for a FULL wave (round 3: the tail queue, pt_kernel.hpp PT_TAILQ; before it a third
//    of the lanes idled through that tail and a minority material's branch ran in every iteration).  Alternatives built and measured on MI355X:
//    a lane pool with vote-driven batched shading (516 vs 654 Msamples/s), one merged shadow+closest traversal loop
//    per iteration (670 vs 851), packed-f32 slab tests (-5 %): slower.  Persistent traversal with dynamic ray fetch
//    (wave-local ray batches): 1.16-1.55x on the stand-alone traversal kernel for
//    incoherent rays, 0.6x for coherent ones — not enough to pay for streaming path state through HBM;
//  * shadow rays use deferred, dense triangle tests (trace_any_deferred, pt_device.hpp): lanes only walk nodes and
//    queue (triangle, lane) pairs in an LDS ring, the wave tests 64 pairs at a time (any-hit is order independent).
//    Measured on C2: any-hit triangle steps per wave iteration 24 at 3.7 % lane use -> 1.8 at 72 %, +4-5 % Msamples/s;
//  * measured and dropped: two work items in flight per wave (a lane that finished its pixel starts the next tile's instead of
//    idling; lanes busy at shading 89 % -> 96 %, but the extra per-lane state spills and the hash table had to leave LDS:
//    -6 % at one GPU, +-0 on a 1/8 shard), a per-lane cache of the in-tile Sobol digits (not wave-uniform: -3 %);
//  * BVH traversal keeps the per-lane stack in LDS (stack[level][lane], conflict-free) and the
//    MurmurHash(dimension, seed) table of the Sobol sampler in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_kernel.hpp"

namespace pt {

// Sensor::to_rgb (sensor.rs:81-88) + ReinhardToneMap (tone_map.rs:20-28) + sRGB OETF (eotf.rs:54-61)
__global__ void resolve_kernel(const float* __restrict__ accum, uint32_t n_values, uint32_t spp, float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t stride = gridDim.x * blockDim.x;
    for (; i < n_values; i += stride) {
        float c = accum[i] / (float)spp;
        c = fmaxf(c, 0.0f);
        c = c / (1.0f + c);
        out[i] = srgb_oetf(c);
    }
}

__global__ void probe_sobol_kernel(uint32_t width, uint32_t seed, uint32_t log2_spp, uint32_t nb4, const uint32_t* __restrict__ xys, uint32_t n,
                                   const uint8_t* __restrict__ pattern, uint32_t n_pat, uint32_t per, uint32_t* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // no LDS hash table here: dim_hash falls back to computing the MurmurHash when the pointer table is absent
    SamplerCtx c{1u, seed, log2_spp, nb4, width, nullptr, nullptr, 0u, 0u};
    Sampler s;
    sampler_start(s, c, xys[3 * i], xys[3 * i + 1], xys[3 * i + 2]);
    uint32_t* o = out + (size_t)i * per;
    for (uint32_t k = 0; k < n_pat; ++k) {
        if (pattern[k] == '2') {
            uint64_t si = sobol_sample_index(s.morton, s.dimension, log2_spp, nb4);
            s.dimension += 2;
            uint64_t h = murmur_dim_seed(s.dimension, seed);
            *o++ = fast_owen(sobol_dim0(si), (uint32_t)h);
            *o++ = fast_owen(sobol_dim1(si), (uint32_t)(h >> 32));
        } else {
            uint64_t si = sobol_sample_index(s.morton, s.dimension, log2_spp, nb4);
            s.dimension += 1;
            uint64_t h = murmur_dim_seed(s.dimension, seed);
            *o++ = fast_owen(sobol_dim0(si), (uint32_t)h);
        }
    }
}

__global__ __launch_bounds__(64) void probe_intersect_kernel(DevScene sc, const float* __restrict__ o, const float* __restrict__ d, uint32_t n,
                                                             float* __restrict__ out_t, uint32_t* __restrict__ out_inst, uint32_t* __restrict__ out_tri,
                                                             float* __restrict__ out_n) {
    __shared__ uint32_t s_stack[STACK_DEPTH * 64];
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    StatCounters st{};
    Hit h{};
    f3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    if (trace_closest<false>(sc, ro, rd, 3.402823466e+38f, s_stack + threadIdx.x, h, st)) {
        Surface sf = load_surface(sc, h, rd);
        const float4* q = (const float4*)(sc.shade + h.tri);
        float4 e = q[4], f = q[5];
        out_t[i] = h.t; out_inst[i] = __float_as_uint(e.w); out_tri[i] = __float_as_uint(f.z);
        if (out_n) { out_n[3 * i] = sf.ng.x; out_n[3 * i + 1] = sf.ng.y; out_n[3 * i + 2] = sf.ng.z; }
    } else {
        out_t[i] = -1.0f; out_inst[i] = 0xffffffffu; out_tri[i] = 0xffffffffu;
        if (out_n) { out_n[3 * i] = 0; out_n[3 * i + 1] = 0; out_n[3 * i + 2] = 0; }
    }
}

// ref_sincosf (pt_device.hpp -> pt_libm.hpp) for the floats with bit patterns first + i * stride: mi355pt_probe_sincos compares them with the host's libm
__global__ void probe_sincos_kernel(uint32_t first, uint32_t stride, uint32_t n, float* __restrict__ out_s, float* __restrict__ out_c) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c;
    ref_sincosf(__uint_as_float(first + i * stride), &s, &c);
    out_s[i] = s; out_c[i] = c;
}
__global__ __launch_bounds__(64) void probe_occluded_kernel(DevScene sc, const float* __restrict__ o, const float* __restrict__ d,
                                                            const float* __restrict__ tmax, uint32_t n, uint8_t* __restrict__ out) {
    __shared__ uint32_t s_stack[STACK_DEPTH * 64];
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    StatCounters st{};
    f3 ro = mk3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    out[i] = trace_any<false>(sc, ro, rd, tmax[i], s_stack + threadIdx.x, st) ? 1 : 0;
}

// Multi-device gather (mi355pt_render_multi): a device's shard of the frame as a COMPACT film — its 8x8 tiles in shard order (tile k of the
// shard = frame tile shard_index + k * shard_count), 64 pixels x 3 floats each, pixels outside the frame 0 — so that 1/N of the film
// crosses xGMI per peer instead of the whole frame; and the inverse on the gathering device (the shards' tiles are disjoint: plain stores).
__global__ void film_pack_kernel(const float* __restrict__ film, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_index, uint32_t shard_count,
                                 uint32_t n_tiles, float* __restrict__ packed) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= n_tiles) return;
    const uint32_t tile = shard_index + k * shard_count;
    const uint32_t px = (tile % tiles_x) * 8u + (lane & 7u), py = (tile / tiles_x) * 8u + (lane >> 3);
    const bool in = px < width && py < height;
    const size_t o = ((size_t)py * width + px) * 3, q = ((size_t)k * 64u + lane) * 3u;
    packed[q] = in ? film[o] : 0.0f; packed[q + 1] = in ? film[o + 1] : 0.0f; packed[q + 2] = in ? film[o + 2] : 0.0f;
}
__global__ void film_unpack_kernel(float* __restrict__ film, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_index, uint32_t shard_count,
                                   uint32_t n_tiles, const float* __restrict__ packed) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= n_tiles) return;
    const uint32_t tile = shard_index + k * shard_count;
    const uint32_t px = (tile % tiles_x) * 8u + (lane & 7u), py = (tile / tiles_x) * 8u + (lane >> 3);
    if (px >= width || py >= height) return;
    const size_t o = ((size_t)py * width + px) * 3, q = ((size_t)k * 64u + lane) * 3u;
    film[o] = packed[q]; film[o + 1] = packed[q + 1]; film[o + 2] = packed[q + 2];
}

// adds the per-chunk film tiles of a split launch to the film, in chunk order (one thread per pixel of each tile of the shard)
__global__ void combine_kernel(DevCamera cam, DevParams prm, const float* __restrict__ partial, float* __restrict__ accum, uint32_t n_tiles) {
    const uint32_t tile_k = blockIdx.x, lane = threadIdx.x;
    if (tile_k >= n_tiles) return;
    const uint32_t tile = prm.shard_index + tile_k * prm.shard_count;
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

// the instrumented variants, both generic-mode kernels (launch_plan.hpp select_kernel says which scenes take which); nullptr: no such variant
static PtKernel instrumented_kernel(uint32_t set) {
    if (set == (FEAT_STD & ~FEAT_CC)) return pt_kernel<true, FEAT_STD & ~FEAT_CC, MODE_GENERIC>;
    return set == FEAT_ALL ? pt_kernel<true, FEAT_ALL, MODE_GENERIC> : nullptr;
}

}  // namespace pt

// the production kernels of this unit: the generic mode (strategy and sampler read from DevParams), both feature-set classes
PT_KERNELS_CC(MODE_GENERIC)
PT_KERNELS_PLAIN(MODE_GENERIC)

namespace pt {

__global__ void combine_tiles_kernel(DevCamera cam, DevParams prm, const float* __restrict__ partial, float* __restrict__ accum, uint32_t n_list);   // pt_kernels_tiles.hip

// ---------------------------------------------------------------------------------------------
// launch wrappers (host side, declared in launch.hpp for api.cpp / api_debug.cpp)
// ---------------------------------------------------------------------------------------------
// The instantiation a key (launch_plan.hpp select_kernel) names, wherever it is compiled; nullptr: there is none (an instrumented tile-list
// kernel, a set that is not in the list of its class).  The ONE place a launch and its occupancy query take their kernel from.
static PtKernel find_pt_kernel(const KernelKey& key) {
    if (key.stats) return !key.tiles && key.mode == MODE_GENERIC ? instrumented_kernel(key.set) : nullptr;
    // [MODE_*][tile list][clearcoat class]: one entry per translation unit's share of the production kernels
    using Unit = PtKernel (*)(uint32_t set);
#define PT_UNITS_OF(M) {{production_kernel<false, M, false>, production_kernel<false, M, true>}, {production_kernel<true, M, false>, production_kernel<true, M, true>}}
    static const Unit units[MODE_COUNT][2][2] = {PT_UNITS_OF(MODE_GENERIC), PT_UNITS_OF(MODE_MIS_SOBOL), PT_UNITS_OF(MODE_NEE_SOBOL), PT_UNITS_OF(MODE_PT)};
#undef PT_UNITS_OF
    static_assert(MODE_GENERIC == 0 && MODE_MIS_SOBOL == 1 && MODE_NEE_SOBOL == 2 && MODE_PT == 3, "units[] is indexed by MODE");
    return key.mode < MODE_COUNT ? units[key.mode][key.tiles ? 1 : 0][(key.set & FEAT_CC) ? 1 : 0](key.set) : nullptr;
}
hipError_t launch_pt(const KernelKey& key, const DevScene& sc, const DevCamera& cam, const DevParams& prm, uint32_t n_tiles, const uint64_t* d_hash,
                     float* d_accum, float* d_partial, unsigned* d_counter, DevStats* d_stats, int grid, hipStream_t stream, const PathOut& pout,
                     float* d_defer) {
    const PtKernel kernel = find_pt_kernel(key);
    if (!kernel) return hipErrorInvalidDeviceFunction;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, stream, sc, cam, prm, d_hash, d_accum, d_partial, d_counter, d_stats, pout, (float4*)d_defer);
    if (prm.chunks > 1)
        hipLaunchKernelGGL(key.tiles ? combine_tiles_kernel : combine_kernel, dim3(n_tiles), dim3(64), 0, stream, cam, prm, (const float*)d_partial, d_accum, n_tiles);
    return hipGetLastError();
}
hipError_t launch_film_pack(const float* film, uint32_t w, uint32_t h, uint32_t shard_index, uint32_t shard_count, uint32_t n_tiles, float* packed, hipStream_t stream) {
    if (n_tiles) hipLaunchKernelGGL(film_pack_kernel, dim3(n_tiles), dim3(64), 0, stream, film, w, h, (w + 7u) / 8u, shard_index, shard_count, n_tiles, packed);
    return hipGetLastError();
}
hipError_t launch_film_unpack(float* film, uint32_t w, uint32_t h, uint32_t shard_index, uint32_t shard_count, uint32_t n_tiles, const float* packed, hipStream_t stream) {
    if (n_tiles) hipLaunchKernelGGL(film_unpack_kernel, dim3(n_tiles), dim3(64), 0, stream, film, w, h, (w + 7u) / 8u, shard_index, shard_count, n_tiles, packed);
    return hipGetLastError();
}
hipError_t launch_resolve(const float* d_accum, uint32_t n_values, uint32_t spp, float* d_out, hipStream_t stream) {
    int grid = (int)std::min<uint32_t>((n_values + 255) / 256, 2048u);
    hipLaunchKernelGGL(resolve_kernel, dim3(grid), dim3(256), 0, stream, d_accum, n_values, spp, d_out);
    return hipGetLastError();
}
hipError_t launch_probe_sobol(uint32_t width, uint32_t seed, uint32_t log2_spp, uint32_t nb4, const uint32_t* d_xys, uint32_t n,
                              const uint8_t* d_pat, uint32_t n_pat, uint32_t per, uint32_t* d_out, hipStream_t stream) {
    hipLaunchKernelGGL(probe_sobol_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, width, seed, log2_spp, nb4, d_xys, n, d_pat, n_pat, per, d_out);
    return hipGetLastError();
}
hipError_t launch_probe_intersect(const DevScene& sc, const float* o, const float* d, uint32_t n, float* t, uint32_t* inst, uint32_t* tri, float* nrm,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(probe_intersect_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, sc, o, d, n, t, inst, tri, nrm);
    return hipGetLastError();
}
hipError_t launch_probe_sincos(uint32_t first, uint32_t stride, uint32_t n, float* out_s, float* out_c, hipStream_t stream) {
    hipLaunchKernelGGL(probe_sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, first, stride, n, out_s, out_c);
    return hipGetLastError();
}
hipError_t launch_probe_occluded(const DevScene& sc, const float* o, const float* d, const float* tmax, uint32_t n, uint8_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(probe_occluded_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, sc, o, d, tmax, n, out);
    return hipGetLastError();
}


uint64_t host_murmur_dim_seed(uint32_t dimension, uint32_t seed) { return murmur_dim_seed(dimension, seed); }
// the queue memory a resident wave of the kernel launch_pt takes for `key` uses (pt_kernel.hpp queue_bytes_per_wave: the kernel's own stride)
size_t query_defer_bytes_per_wave(const KernelKey& key) { return queue_bytes_per_wave(key.stats, key.set, key.mode); }
// resident 64-thread blocks (= waves) on the current device of the kernel instantiation launch_pt takes for `key`, through the same lookup:
// the persistent grid size.  The MODE specialisations are separate translation units with their own backend flags, so their register
// counts — and with them the occupancy — need not be those of the generic variant.  Cached per scene and device (api.cpp LaunchCtx).
int query_resident_waves(const KernelKey& key) {
    const PtKernel kernel = find_pt_kernel(key);
    return kernel ? resident_waves_of(kernel) : resident_waves_per_device(0);
}
}  // namespace pt
