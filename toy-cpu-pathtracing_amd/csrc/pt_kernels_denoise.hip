// The denoiser of include/mi355pt_denoise.h — an edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) over the linear film of a
// path renderer, guided by the albedo and shading-normal films — as two plain HIP kernels for gfx950.  EXTENSION, no reference counterpart.
//
// Records.  The prepass turns the three W x H x 3 films of sums into 16-byte records in the caller's scratch, one array per kind:
//     irr  (irr.x, irr.y, irr.z, 0)            two arrays, read and written alternately by the levels
//     nrm  (n.x, n.y, n.z, background flag)    the flag is the WORD 1 on a background pixel, 0 elsewhere
//     alb  (a.x, a.y, a.z, 0)
// so a level reads 48 B and writes 16 B per pixel that MUST move (64 B per pixel and level), and every tap of a wave is one coalesced
// dwordx4 load per array for any step: a wave covers 64 consecutive x of one row, a 64 x 4 block four rows whose taps share rows in L1 / L2.
// A background pixel's irr record holds c itself (never divided by the albedo): the levels copy it through and the last one writes it out.
//
// Arithmetic of a tap: |t(x_p) - t(x_q)| = |x_p - x_q| / ((1 + x_p)(1 + x_q)) per channel, with one hardware reciprocal per channel of the
// tap (the centre's are taken once) instead of a division — also free of the cancellation of t(x_p) - t(x_q) —; the three sigma factors
// arrive premultiplied by log2(e), so that the weight is h[dx] h[dy] exp2(-d'): ONE v_exp_f32 per tap.  Taps outside the image and background
// taps load the centre's records again (a cached address, no branch) and get the factor 0 into their weight, so that the taps' loads can be
// in flight together.  One IEEE division per channel and pixel at the end.  No atomics, a fixed summation order: two runs are bit-equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"

namespace pt {

namespace {

__device__ __forceinline__ float dn_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

__global__ __launch_bounds__(256) void denoise_prepass_kernel(const float* __restrict__ beauty, const float* __restrict__ albedo,
                                                              const float* __restrict__ normal, float spp_b, float spp_a, float spp_n,
                                                              float albedo_eps, size_t n_pixels, float4* __restrict__ irr,
                                                              float4* __restrict__ nrm, float4* __restrict__ alb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n_pixels; i += stride) {
        float cx = dn_clean(beauty[3 * i], spp_b), cy = dn_clean(beauty[3 * i + 1], spp_b), cz = dn_clean(beauty[3 * i + 2], spp_b);
        bool bg = false;
        if (normal != nullptr) {
            const float n0 = normal[3 * i], n1 = normal[3 * i + 1], n2 = normal[3 * i + 2];
            bg = n0 == 0.0f && n1 == 0.0f && n2 == 0.0f;                 // every sample missed (misses add 0, hits add n * 0.5 + 0.5)
            nrm[i] = make_float4(2.0f * (n0 / spp_n) - 1.0f, 2.0f * (n1 / spp_n) - 1.0f, 2.0f * (n2 / spp_n) - 1.0f, __uint_as_float(bg ? 1u : 0u));
        }
        if (albedo != nullptr) {
            const float ax = dn_clip0(albedo[3 * i], spp_a), ay = dn_clip0(albedo[3 * i + 1], spp_a), az = dn_clip0(albedo[3 * i + 2], spp_a);
            alb[i] = make_float4(ax, ay, az, 0.0f);
            if (!bg) { cx = cx / (ax + albedo_eps); cy = cy / (ay + albedo_eps); cz = cz / (az + albedo_eps); }
        }
        irr[i] = make_float4(cx, cy, cz, 0.0f);
    }
}

struct DnLevel {
    uint32_t width, height, blocks_x, step;
    float k_color, k_normal, k_albedo;     // log2(e) * (4^i / sigma_color^2, 1 / sigma_normal^2, 1 / sigma_albedo^2)
    float albedo_eps;
};

// One level.  LAST: the remodulation and the background copy are fused in, and the result goes to the W x H x 3 film `out` instead of irr_out.
template <bool HAS_N, bool HAS_A, bool LAST>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_level_kernel(const float4* __restrict__ irr_in, const float4* __restrict__ nrm,
                                                                                const float4* __restrict__ alb, float4* __restrict__ irr_out,
                                                                                float* __restrict__ out, DnLevel lv) {
    const uint32_t bx = blockIdx.x % lv.blocks_x, by = blockIdx.x / lv.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= lv.width || y >= lv.height) return;
    const size_t p = (size_t)y * lv.width + x;
    const float4 ip = irr_in[p];
    float4 np = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ap = np;
    if constexpr (HAS_N) np = nrm[p];
    if constexpr (HAS_A) ap = alb[p];
    float rx = ip.x, ry = ip.y, rz = ip.z;                             // a background pixel keeps its value
    const bool bg = HAS_N && __float_as_uint(np.w) != 0u;
    if (!bg) {
        const float tpx = dn_rcp(1.0f + ip.x), tpy = dn_rcp(1.0f + ip.y), tpz = dn_rcp(1.0f + ip.z);
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
        // all 25 taps unrolled: the compiler hoists the loads of many taps above the arithmetic (126 - 132 VGPRs with both guides, 3 - 4
        // waves per SIMD, no scratch).  That beat the rows rolled (`#pragma unroll 1` here: 60 VGPRs, 8 waves per SIMD, the loads of 5 taps
        // in flight) when the two builds alternated on one MI355X: profiles/denoise_ab.json, DESIGN.md 4.7
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint32_t oy = (uint32_t)(j < 2 ? 2 - j : j - 2) * lv.step;
            const bool vy = j < 2 ? y >= oy : lv.height - y > oy;     // (no sum that could wrap: y < height)
            const size_t row = j < 2 ? p - (size_t)oy * lv.width : p + (size_t)oy * lv.width;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const uint32_t ox = (uint32_t)(i < 2 ? 2 - i : i - 2) * lv.step;
                const bool inside = vy && (i < 2 ? x >= ox : lv.width - x > ox);
                const size_t q = inside ? (i < 2 ? row - ox : row + ox) : p;      // an index inside the frame in every case
                const float4 iq = irr_in[q];
                const float ex = (ip.x - iq.x) * (tpx * dn_rcp(1.0f + iq.x));
                const float ey = (ip.y - iq.y) * (tpy * dn_rcp(1.0f + iq.y));
                const float ez = (ip.z - iq.z) * (tpz * dn_rcp(1.0f + iq.z));
                float d = lv.k_color * (ex * ex + ey * ey + ez * ez);
                bool use = inside;
                if constexpr (HAS_N) {
                    const float4 nq = nrm[q];
                    const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
                    d = fmaf(lv.k_normal, dx * dx + dy * dy + dz * dz, d);
                    use = use && __float_as_uint(nq.w) == 0u;
                }
                if constexpr (HAS_A) {
                    const float4 aq = alb[q];
                    const float dx = ap.x - aq.x, dy = ap.y - aq.y, dz = ap.z - aq.z;
                    d = fmaf(lv.k_albedo, dx * dx + dy * dy + dz * dz, d);
                }
                // the weight of an unused tap is 0 by a FACTOR, not by a select around the tap: a select lets the compiler branch around the
                // tap's loads on the flag, which chains two memory round trips per tap.  0 * exp2(-d) is 0 as long as d is no NaN: the header
                // asks for finite guide films, the prepass cleans the beauty, the host keeps the k factors finite, and an infinite d gives
                // exp2(-inf) = 0.  With non-finite guides (or an irr that overflows f32) the result is unspecified, here as in the header
                const float w = (use ? dn_h5(i) * dn_h5(j) : 0.0f) * __builtin_amdgcn_exp2f(-d);
                sw += w;
                sx = fmaf(w, iq.x, sx); sy = fmaf(w, iq.y, sy); sz = fmaf(w, iq.z, sz);
            }
        }
        rx = sx / sw; ry = sy / sw; rz = sz / sw;                       // the centre tap (d = 0, w = 9/64) makes sw > 0
    }
    if constexpr (LAST) {
        if (HAS_A && !bg) { rx = rx * (ap.x + lv.albedo_eps); ry = ry * (ap.y + lv.albedo_eps); rz = rz * (ap.z + lv.albedo_eps); }
        out[3 * p] = rx; out[3 * p + 1] = ry; out[3 * p + 2] = rz;
    } else {
        irr_out[p] = make_float4(rx, ry, rz, 0.0f);
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api.cpp, which has checked every argument) ----
size_t denoise_scratch_bytes(uint32_t width, uint32_t height) {
    const unsigned __int128 b = (unsigned __int128)width * height * 64u;
    return b > (unsigned __int128)SIZE_MAX ? 0 : (size_t)b;
}
// blocks of one level launch; 0 = more than a grid holds
uint32_t denoise_grid_blocks(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)((width + (uint64_t)DN_BLOCK_X - 1) / DN_BLOCK_X) * ((height + (uint64_t)DN_BLOCK_Y - 1) / DN_BLOCK_Y);
    return n > 0x7fffffffull ? 0u : (uint32_t)n;
}

hipError_t launch_denoise(const float* d_beauty, uint32_t spp_b, const float* d_albedo, uint32_t spp_a, const float* d_normal, uint32_t spp_n,
                          uint32_t width, uint32_t height, uint32_t levels, float sigma_color, float sigma_normal, float sigma_albedo,
                          float albedo_eps, void* d_scratch, float* d_out, hipStream_t stream) {
    const size_t n_pixels = (size_t)width * height;
    float4* irr[2] = {(float4*)d_scratch, (float4*)d_scratch + n_pixels};
    float4* nrm = (float4*)d_scratch + 2 * n_pixels;
    float4* alb = (float4*)d_scratch + 3 * n_pixels;
    const int pre_grid = (int)std::min<size_t>((n_pixels + 255) / 256, 4096);
    hipLaunchKernelGGL(denoise_prepass_kernel, dim3(pre_grid), dim3(256), 0, stream, d_beauty, d_albedo, d_normal, (float)spp_b, (float)spp_a,
                       (float)spp_n, albedo_eps, n_pixels, irr[0], nrm, alb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double log2e = 1.4426950408889634;
    // a factor that overflows f32 (a sigma near 1e-20) stays the largest float: an infinite one times the centre tap's distance 0 is a NaN
    auto finite_f32 = [](double k) { return (float)std::min(k, (double)FLT_MAX); };
    DnLevel lv{width, height, (uint32_t)(((uint64_t)width + DN_BLOCK_X - 1) / DN_BLOCK_X), 1u, 0.0f, finite_f32(log2e / ((double)sigma_normal * sigma_normal)),
               finite_f32(log2e / ((double)sigma_albedo * sigma_albedo)), albedo_eps};
    const dim3 grid(denoise_grid_blocks(width, height)), block(DN_BLOCK_X, DN_BLOCK_Y);
    for (uint32_t i = 0; i < levels; ++i) {
        lv.step = 1u << i;
        lv.k_color = finite_f32(log2e * (double)(1u << (2u * i)) / ((double)sigma_color * sigma_color));
        const float4* in = irr[i & 1u];
        float4* out = irr[(i & 1u) ^ 1u];
        const bool last = i + 1 == levels;
#define PT_DN_LAUNCH(N, A)                                                                                                                  \
    do {                                                                                                                                    \
        if (last) hipLaunchKernelGGL((denoise_level_kernel<N, A, true>), grid, block, 0, stream, in, nrm, alb, out, d_out, lv);             \
        else hipLaunchKernelGGL((denoise_level_kernel<N, A, false>), grid, block, 0, stream, in, nrm, alb, out, d_out, lv);                 \
    } while (0)
        if (d_normal != nullptr && d_albedo != nullptr) PT_DN_LAUNCH(true, true);
        else if (d_normal != nullptr) PT_DN_LAUNCH(true, false);
        else if (d_albedo != nullptr) PT_DN_LAUNCH(false, true);
        else PT_DN_LAUNCH(false, false);
#undef PT_DN_LAUNCH
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
