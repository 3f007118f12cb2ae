// The denoiser of include/mi355pt_denoise_var.h — an a-trous wavelet filter whose luminance edge stop is scaled by the per-pixel variance
// that the film and the half film give (in the manner of SVGF, Schied et al., HPG 2017), guided by the albedo and shading-normal films — as
// two plain HIP kernels for gfx950.  EXTENSION, no reference counterpart; a second filter beside pt_kernels_denoise.hip, whose shape it
// keeps: one thread per pixel, 64 x 4 blocks, 16-byte records, every tap loaded unconditionally with the weight 0 by a factor.
//
// Records, one array per kind in the caller's scratch:
//     irr  (irr.x, irr.y, irr.z, var)          two arrays, read and written alternately by the levels
//     nrm  (n.x, n.y, n.z, background flag)    the flag is the WORD 1 on a background pixel, 0 elsewhere
//     alb  (a.x, a.y, a.z, 0)
// The variance rides in the word of the irr record that the other filter leaves 0, so a level still moves 64 B per pixel.  A background
// pixel's irr record holds (c, -1): c is copied through the levels and written out by the last one, and the NEGATIVE variance word tells
// the 3 x 3 filter G below that the pixel is background without a load of its normal record (a variance is never negative; a background
// tap's weight is 0 by its normal record's flag, as in the other filter, so the -1 never reaches a sum).
//
// sd_p = sqrt(G(var)_p) comes from eight extra one-word loads at distance 1 in the level kernel itself — unconditional, at indices clamped
// to the frame; rows the block's own taps of level 0 touch and that stay in L1 / L2 on the others — instead of a pass of its own per level (which would read 16 B and write 4 B per
// pixel and level more, and launch once more).  G's weights are taken as 1 2 1; 2 4 2; 1 2 1: the / 16 cancels in the quotient, and
// scaling by a power of two is exact.
//
// Arithmetic of a tap: |lum(irr_p) - lum(irr_q)| / (sigma_lum sd_p + lum_eps) = |s_p - s_q| k_p with s = (x + y) + z and
// k_p = (log2(e) / 3) / (sigma_lum sd_p + lum_eps), one IEEE division per pixel and level; the two guide factors arrive premultiplied by
// log2(e), so that the weight is h[dx] h[dy] exp2(-d'): ONE v_exp_f32 per tap.  No atomics, a fixed summation order: two runs are bit-equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"

namespace pt {

namespace {

__device__ __forceinline__ float dv_lum(float x, float y, float z) { return ((x + y) + z) / 3.0f; }

// d_tile_spp == nullptr: every pixel has `spp_b` samples; otherwise the count of the pixel's 8 x 8 tile (tiles_x tiles per row)
__global__ __launch_bounds__(256) void denoise_var_prepass_kernel(const float* __restrict__ beauty, const float* __restrict__ half,
                                                                  const uint32_t* __restrict__ tile_spp, const float* __restrict__ albedo,
                                                                  const float* __restrict__ normal, uint32_t spp_b, float spp_a, float spp_n,
                                                                  float albedo_eps, uint32_t width, uint32_t tiles_x, size_t n_pixels,
                                                                  float4* __restrict__ irr, float4* __restrict__ nrm, float4* __restrict__ alb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n_pixels; i += stride) {
        uint32_t n = spp_b;
        if (tile_spp != nullptr) {
            const size_t y = i / width, x = i - y * width;
            n = tile_spp[(y >> 3) * tiles_x + (x >> 3)];
        }
        const float nf = (float)n, hf = (float)(n >> 1);
        float c[3], c1[3], c2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float b = beauty[3 * i + k], h = half[3 * i + k];
            c[k] = dn_clean(b, nf); c1[k] = dn_clean(h, hf); c2[k] = dn_clean(b - h, hf);
        }
        bool bg = false;
        if (normal != nullptr) {
            const float n0 = normal[3 * i], n1 = normal[3 * i + 1], n2 = normal[3 * i + 2];
            bg = n0 == 0.0f && n1 == 0.0f && n2 == 0.0f;                 // every sample missed (misses add 0, hits add n * 0.5 + 0.5)
            nrm[i] = make_float4(2.0f * (n0 / spp_n) - 1.0f, 2.0f * (n1 / spp_n) - 1.0f, 2.0f * (n2 / spp_n) - 1.0f, __uint_as_float(bg ? 1u : 0u));
        }
        if (albedo != nullptr) {
            const float a[3] = {dn_clip0(albedo[3 * i], spp_a), dn_clip0(albedo[3 * i + 1], spp_a), dn_clip0(albedo[3 * i + 2], spp_a)};
            alb[i] = make_float4(a[0], a[1], a[2], 0.0f);
            if (!bg) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float den = a[k] + albedo_eps;
                    c[k] = c[k] / den; c1[k] = c1[k] / den; c2[k] = c2[k] / den;
                }
            }
        }
        const float dl = (dv_lum(c1[0], c1[1], c1[2]) - dv_lum(c2[0], c2[1], c2[2])) / 2.0f;
        irr[i] = make_float4(c[0], c[1], c[2], bg ? -1.0f : dl * dl);
    }
}

struct DvLevel {
    uint32_t width, height, blocks_x, step;
    float sigma_lum, lum_eps;
    float k_normal, k_albedo;              // log2(e) * (1 / sigma_normal^2, 1 / sigma_albedo^2)
    float albedo_eps;
};

// One level.  LAST: the remodulation and the background copy are fused in, and the result goes to the W x H x 3 film `out` instead of irr_out.
template <bool HAS_N, bool HAS_A, bool LAST>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void denoise_var_level_kernel(const float4* __restrict__ irr_in, const float4* __restrict__ nrm,
                                                                                    const float4* __restrict__ alb, float4* __restrict__ irr_out,
                                                                                    float* __restrict__ out, DvLevel lv) {
    const uint32_t bx = blockIdx.x % lv.blocks_x, by = blockIdx.x / lv.blocks_x;
    const uint32_t x = bx * DN_BLOCK_X + threadIdx.x, y = by * DN_BLOCK_Y + threadIdx.y;
    if (x >= lv.width || y >= lv.height) return;
    const size_t p = (size_t)y * lv.width + x;
    const float4 ip = irr_in[p];
    float4 np = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ap = np;
    if constexpr (HAS_N) np = nrm[p];
    if constexpr (HAS_A) ap = alb[p];
    float rx = ip.x, ry = ip.y, rz = ip.z, rv = ip.w;                  // a background pixel keeps its record
    const bool bg = HAS_N && __float_as_uint(np.w) != 0u;
    if (!bg) {
        // G(var)_p over the in-frame, non-background pixels of the 3 x 3 around p (the centre is both: gw >= 4).  A neighbour's row and
        // column are CLAMPED to the frame, so all nine one-word loads are unconditional and issue together; a neighbour that the clamp moved
        // (it is out of frame) or that is background takes the weight 0 and the value 0 by selects on the loaded word, not around the load
        const uint32_t gx[3] = {x - (x >= 1u ? 1u : 0u), x, x + (lv.width - x > 1u ? 1u : 0u)};
        const uint32_t gy[3] = {y - (y >= 1u ? 1u : 0u), y, y + (lv.height - y > 1u ? 1u : 0u)};
        float gv[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t row = (size_t)gy[j] * lv.width;
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[3 * j + i] = (i == 1 && j == 1) ? ip.w : irr_in[row + gx[i]].w;
        }
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const bool inside = gx[i] + 1u == x + (uint32_t)i && gy[j] + 1u == y + (uint32_t)j;   // the clamp did not move it
                const float vq = gv[3 * j + i];
                const bool use = inside && vq >= 0.0f;
                const float k = use ? (float)((i == 1 ? 2 : 1) * (j == 1 ? 2 : 1)) : 0.0f;
                gs = fmaf(k, use ? vq : 0.0f, gs);                            // k vq is exact: the fma rounds what the sum rounds
                gw += k;
            }
        }
        const float sd = sqrtf(gs / gw);
        // (a lum_eps so small that the quotient overflows stays the largest float: an infinite factor times the centre tap's distance 0 is a NaN)
        const float kp = fminf((float)(1.4426950408889634 / 3.0) / (lv.sigma_lum * sd + lv.lum_eps), FLT_MAX);
        const float sp = (ip.x + ip.y) + ip.z;
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
        // all 25 taps unrolled, as in pt_kernels_denoise.hip: the loads of many taps are in flight together
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
                float d = fabsf(sp - ((iq.x + iq.y) + iq.z)) * kp;
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
                // the weight of an unused tap is 0 by a FACTOR, not by a select around the tap (pt_kernels_denoise.hip has the reason); d is no
                // NaN: the guides are finite, the prepass cleans both films, kp and the k factors are finite
                const float w = (use ? dn_h5(i) * dn_h5(j) : 0.0f) * __builtin_amdgcn_exp2f(-d);
                sw += w;
                sx = fmaf(w, iq.x, sx); sy = fmaf(w, iq.y, sy); sz = fmaf(w, iq.z, sz);
                sv = fmaf(w * w, iq.w, sv);
            }
        }
        rx = sx / sw; ry = sy / sw; rz = sz / sw;                       // the centre tap (d = 0, w = 9/64) makes sw > 0
        if constexpr (!LAST) rv = sv / (sw * sw);
    }
    if constexpr (LAST) {
        if (HAS_A && !bg) { rx = rx * (ap.x + lv.albedo_eps); ry = ry * (ap.y + lv.albedo_eps); rz = rz * (ap.z + lv.albedo_eps); }
        out[3 * p] = rx; out[3 * p + 1] = ry; out[3 * p + 2] = rz;
    } else {
        irr_out[p] = make_float4(rx, ry, rz, rv);
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api.cpp, which has checked every argument) ----
// the four 16-byte records per pixel of pt_kernels_denoise.hip: the variance takes the word that is 0 there
size_t denoise_var_scratch_bytes(uint32_t width, uint32_t height) { return denoise_scratch_bytes(width, height); }

hipError_t launch_denoise_var(const float* d_beauty, const float* d_half, uint32_t spp_b, const uint32_t* d_tile_spp, const float* d_albedo, uint32_t spp_a,
                              const float* d_normal, uint32_t spp_n, uint32_t width, uint32_t height, uint32_t levels, float sigma_lum, float sigma_normal,
                              float sigma_albedo, float albedo_eps, float lum_eps, void* d_scratch, float* d_out, hipStream_t stream) {
    const size_t n_pixels = (size_t)width * height;
    float4* irr[2] = {(float4*)d_scratch, (float4*)d_scratch + n_pixels};
    float4* nrm = (float4*)d_scratch + 2 * n_pixels;
    float4* alb = (float4*)d_scratch + 3 * n_pixels;
    const int pre_grid = (int)std::min<size_t>((n_pixels + 255) / 256, 4096);
    hipLaunchKernelGGL(denoise_var_prepass_kernel, dim3(pre_grid), dim3(256), 0, stream, d_beauty, d_half, d_tile_spp, d_albedo, d_normal, spp_b, (float)spp_a,
                       (float)spp_n, albedo_eps, width, (uint32_t)(((uint64_t)width + 7u) / 8u), n_pixels, irr[0], nrm, alb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double log2e = 1.4426950408889634;
    // a factor that overflows f32 (a sigma near 1e-20) stays the largest float: an infinite one times the centre tap's distance 0 is a NaN
    auto finite_f32 = [](double k) { return (float)std::min(k, (double)FLT_MAX); };
    DvLevel lv{width, height, (uint32_t)(((uint64_t)width + DN_BLOCK_X - 1) / DN_BLOCK_X), 1u, sigma_lum, lum_eps,
               finite_f32(log2e / ((double)sigma_normal * sigma_normal)), finite_f32(log2e / ((double)sigma_albedo * sigma_albedo)), albedo_eps};
    const dim3 grid(denoise_grid_blocks(width, height)), block(DN_BLOCK_X, DN_BLOCK_Y);
    for (uint32_t i = 0; i < levels; ++i) {
        lv.step = 1u << i;
        const float4* in = irr[i & 1u];
        float4* out = irr[(i & 1u) ^ 1u];
        const bool last = i + 1 == levels;
#define PT_DV_LAUNCH(N, A)                                                                                                                  \
    do {                                                                                                                                    \
        if (last) hipLaunchKernelGGL((denoise_var_level_kernel<N, A, true>), grid, block, 0, stream, in, nrm, alb, out, d_out, lv);         \
        else hipLaunchKernelGGL((denoise_var_level_kernel<N, A, false>), grid, block, 0, stream, in, nrm, alb, out, d_out, lv);             \
    } while (0)
        if (d_normal != nullptr && d_albedo != nullptr) PT_DV_LAUNCH(true, true);
        else if (d_normal != nullptr) PT_DV_LAUNCH(true, false);
        else if (d_albedo != nullptr) PT_DV_LAUNCH(false, true);
        else PT_DV_LAUNCH(false, false);
#undef PT_DV_LAUNCH
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
