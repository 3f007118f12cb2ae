// The robust film of include/mi355pt_robust.h — a per-pixel trimmed mean of K bucket means whose trim comes from their Gini coefficient
// (Buisine, Delepoulle, Renaud: adaptive Median of meaNs, EGSR 2021) — as ONE streaming HIP kernel for gfx950.  EXTENSION, no reference
// counterpart.
//
//   robust_kernel<N, PAIR, POW2>   one thread per pixel, one instantiation per set size N in {2, 4, 8, 16, 32}.  Single output: one set of
//                           N = K buckets; pair output: the N = K / 2 body twice, over the even and over the odd buckets (stride 2).
//                           A register array indexed at run time goes to scratch memory, so every loop over buckets is fully unrolled and
//                           every index is a compile-time constant: the bucket values, luminances and ranks are named registers.  All
//                           3 N loads of a set are issued before the first use and are unconditional — a lane outside the frame clamps its
//                           pixel index and drops the stores.  Ranks by counting: N (N - 1) / 2 compares, each giving one rank to the
//                           larger side (ties to the higher index), which is exactly r_k of the header.  No LDS, no atomics, no scratch.
//                           N = 32 keeps its 96 channel values in registers (166 VGPRs, 3 waves per SIMD).  A second shape, which kept
//                           only luminances and ranks and loaded the buckets again for the output sum, was built and measured on MI355X:
//                           0.270 ms against 0.266 ms for a 1920 x 1080 frame, no gain, so it was removed.
//
// Every float operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls
// no fmaf), divisions are IEEE: every output value is bit-equal to tests/robust_reference.py.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/mi355pt_robust.h"
#include "launch.hpp"

namespace pt {

namespace {

constexpr int RB_BLOCK = 256;

// bucket k of a set whose first bucket starts at `p` (already at the pixel): STRIDE buckets further each
template <int STRIDE>
__device__ __forceinline__ const float* rb_bucket(const float* p, uint64_t frame_floats, int k) { return p + (uint64_t)(k * STRIDE) * frame_floats; }

// step 1.  POW2: spp_bucket is a power of two and a.inv_spp its reciprocal, an exact float — sum * inv_spp and sum / spp are then the same
// real number rounded once, so the same bits, subnormal results included; the product is one instruction where the IEEE division is a dozen
template <bool POW2>
__device__ __forceinline__ float rb_mean(float sum, const RobustArgs& a) {
    const float c = POW2 ? sum * a.inv_spp : sum / a.spp;
    return (c > 0.0f && c <= FLT_MAX) ? c : 0.0f;
}

// steps 1 - 7 of the header over one set; p = the pixel's first float in the set's first bucket
template <int N, int STRIDE, bool POW2>
__device__ __forceinline__ void rb_set(const float* __restrict__ p, uint64_t frame_floats, const RobustArgs& a, float theta[3], uint32_t& t_out) {
    float m[N][3], l[N];
    int r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float* q = rb_bucket<STRIDE>(p, frame_floats, k);
        m[k][0] = q[0]; m[k][1] = q[1]; m[k][2] = q[2];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[k][c] = rb_mean<POW2>(m[k][c], a);
        l[k] = ((m[k][0] + m[k][1]) + m[k][2]) / 3.0f;
        r[k] = 0;
    }
    // l_j <= l_k with j < k: j stands before k (the tie goes to the lower index); otherwise k stands before j
#pragma unroll
    for (int k = 1; k < N; ++k) {
#pragma unroll
        for (int j = 0; j < k; ++j) {
            const bool before = l[j] <= l[k];
            r[k] += before ? 1 : 0;
            r[j] += before ? 0 : 1;
        }
    }
    float S = 0.0f, Q = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        S = S + l[k];
        const float w = (float)(2 * r[k] - (N - 1));
        const float wl = w * l[k];
        Q = Q + wl;
    }
    int t = 0;
    if (a.mode == MI355PT_ROBUST_MOM) t = N / 2 - 1;
    else if (a.mode == MI355PT_ROBUST_GMON) {
        const float den = (float)(N - 1) * S;
        const float G = S > 0.0f ? Q / den : 0.0f;
        const float sg = a.gini_scale * G;
        const float g = fminf(1.0f, fmaxf(0.0f, sg));
        const float tf = floorf(g * (float)(N / 2));
        t = min(N / 2 - 1, (int)tf);
    }
    const uint32_t kept = (uint32_t)(N - 2 * t);
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool keep = (uint32_t)(r[k] - t) < kept;       // t <= r_k < N - t
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = keep ? acc[c] + m[k][c] : acc[c];
    }
    const float kf = (float)kept;
#pragma unroll
    for (int c = 0; c < 3; ++c) theta[c] = acc[c] / kf;
    t_out = (uint32_t)t;
}

template <int N, bool PAIR, bool POW2>
__global__ __launch_bounds__(RB_BLOCK) void robust_kernel(const float* __restrict__ buckets, RobustArgs a, float* __restrict__ out, float* __restrict__ out_half,
                                                          uint8_t* __restrict__ out_trim) {
    const uint64_t i = (uint64_t)blockIdx.x * RB_BLOCK + threadIdx.x;
    const bool inside = i < a.pixels;
    const uint64_t ic = inside ? i : a.pixels - 1u;           // every load is unconditional: a lane outside the frame reads the last pixel
    const uint64_t frame_floats = a.pixels * 3u;
    const float* p = buckets + 3u * ic;
    float th[3], th1[3];
    uint32_t t0 = 0, t1 = 0;
    if constexpr (PAIR) {
        rb_set<N, 2, POW2>(p, frame_floats, a, th, t0);
        rb_set<N, 2, POW2>(p + frame_floats, frame_floats, a, th1, t1);
    } else {
        rb_set<N, 1, POW2>(p, frame_floats, a, th, t0);
    }
    if (!inside) return;
    float* o = out + 3u * i;
    if constexpr (PAIR) {
        float* oh = out_half + 3u * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) { oh[c] = th[c]; o[c] = th[c] + th1[c]; }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = th[c];
    }
    if (out_trim) {
        out_trim[2u * i] = (uint8_t)t0;
        out_trim[2u * i + 1u] = (uint8_t)t1;
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_robust.cpp, which has checked every argument) ----
hipError_t launch_robust_combine(const float* d_buckets, uint32_t n_buckets, const RobustArgs& args, float* d_out, float* d_out_half, uint8_t* d_out_trim,
                                 hipStream_t stream) {
    if (args.pixels == 0 || args.pixels >> 32) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((args.pixels + RB_BLOCK - 1u) / RB_BLOCK)), block(RB_BLOCK);      // fewer than 2^32 pixels: at most 2^24 blocks, one launch
    const bool pair = d_out_half != nullptr, pow2 = args.inv_spp != 0.0f;
#define PT_RB_LAUNCH1(N, PAIR, POW2) hipLaunchKernelGGL((robust_kernel<N, PAIR, POW2>), grid, block, 0, stream, d_buckets, args, d_out, d_out_half, d_out_trim)
#define PT_RB_LAUNCH(N, PAIR)                           \
    do {                                                \
        if (pow2) PT_RB_LAUNCH1(N, PAIR, true);         \
        else PT_RB_LAUNCH1(N, PAIR, false);             \
    } while (0)
#define PT_RB_CASE(K)                                    \
    case K:                                              \
        if (pair) PT_RB_LAUNCH(K / 2, true);             \
        else PT_RB_LAUNCH(K, false);                     \
        break;
    switch (n_buckets) {
        PT_RB_CASE(4)
        PT_RB_CASE(8)
        PT_RB_CASE(16)
        PT_RB_CASE(32)
        default: return hipErrorInvalidValue;      // a missing kernel is an error, never another set size
    }
#undef PT_RB_CASE
#undef PT_RB_LAUNCH
#undef PT_RB_LAUNCH1
    return hipGetLastError();
}

}  // namespace pt
