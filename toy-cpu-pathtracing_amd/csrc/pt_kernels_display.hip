// The display stage of include/mi355pt_display.h — a histogram auto-exposure (the METER) and exposure, tone curve and encoding in one pass (the
// DISPLAY) — as three HIP kernels for gfx950.  EXTENSION, no reference counterpart.
//
//   display_hist_kernel     the meter's first launch: the blocks of display_plan.hpp's plan read the film once, 1024 consecutive pixels per
//                           trip, and count into ONE 258-word histogram per block in LDS with integer ds_add (counts do not depend on the
//                           order).  A constant frame would put all 64 lanes of every wave on one LDS word, and the hardware serialises
//                           same-address atomics: so a wave first peels off the lanes that share the bin of its first live lane — one ballot,
//                           one add of the population count by that lane — and only the others add 1 each.  A uniform wave costs one add,
//                           a wave of 64 different bins one more ballot than the plain form.  Each block stores its 258 counts as a row of
//                           the scratch buffer with plain stores: no global atomics, nothing for the caller to clear.
//   display_finish_kernel   the second launch, ONE block of 1024 threads: four groups of 256 sum a quarter of the (at most 256) rows each, column
//                           by column; the trims come from two prefix sums over the 256 bins, N' and S from integer LDS adds; one thread
//                           takes the mean bin, divides and blends.  (First built with 1024 rows of 256-pixel blocks and one thread doing
//                           the trims serially: 0.11 ms, ten times the first launch; profiles/display_rate.json has what this form takes.)
//   display_kernel          one thread per pixel (REINHARD_EXT needs the pixel's luminance; the others take the same shape), one instantiation
//                           per tone curve and encoding.
//
// Every float operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls
// no fmaf), divisions are IEEE, the sRGB OETF is the resolve's device function: the meter and the linear display are bit-equal to
// tests/display_reference.py, and REINHARD + SRGB with exposure 1 is bit-equal to resolve_kernel (pt_kernels.hip) on a finite non-negative film.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mi355pt_display.h"
#include "display_plan.hpp"
#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_device.hpp"

namespace pt {

namespace {

constexpr float DP_X_MAX = 4294967296.0f;      // 2^32: the cap on the exposed value

__host__ __device__ __forceinline__ float dp_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// h(x) of the header: the Uncharted-2 rational curve (x (A x + CB) + DE) / (x (A x + B) + DF) - E / F over its common denominator, where the
// constant terms cancel exactly: positive terms only, h(0) = 0, no cancellation near 0 (the subtraction as written loses every digit there)
__host__ __device__ __forceinline__ float dp_hable(float x) {
    constexpr float A = 0.15f, B = 0.5f, DF = 0.06f, K1 = 0.056f, K0 = 0.001f;
    const float p = A * x;
    const float n = x * (K1 * p + K0), d = DF * (x * (p + B) + DF);
    return n / d;
}
__device__ __forceinline__ float dp_aces(float x) {
    const float n = x * (2.51f * x + 0.03f), d = x * (2.43f * x + 0.59f) + 0.14f;
    return fminf(fmaxf(n / d, 0.0f), 1.0f);
}

__global__ __launch_bounds__(DISPLAY_METER_BLOCK) void display_hist_kernel(const float* __restrict__ film, uint64_t pixels, uint32_t rows, uint32_t trips, float spp,
                                                                          uint32_t base, uint32_t* __restrict__ scratch) {
    __shared__ uint32_t h[DISPLAY_HIST_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < DISPLAY_HIST_WORDS) h[tid] = 0u;
    __syncthreads();
    for (uint32_t k = 0; k < trips; ++k) {
        const uint64_t i = ((uint64_t)k * rows + blockIdx.x) * DISPLAY_METER_BLOCK + tid;
        const bool valid = i < pixels;
        uint32_t slot = 0u;
        if (valid) {
            const float* f = film + 3 * i;
            const float r = dn_clean(f[0], spp), g = dn_clean(f[1], spp), b = dn_clean(f[2], spp);
            const uint32_t t = __float_as_uint(dp_lum(r, g, b)) >> 20;
            slot = t < base ? 256u : (t >= base + 256u ? 257u : t - base);
        }
        const unsigned long long live = __ballot(valid);
        if (live != 0ull) {                                       // (wave-uniform)
            const int leader = __ffsll((long long)live) - 1;
            const uint32_t lead_slot = (uint32_t)__shfl((int)slot, leader);
            const bool same = valid && slot == lead_slot;
            const unsigned long long peers = __ballot(same);
            if ((int)lane == leader) atomicAdd(&h[lead_slot], (uint32_t)__popcll(peers));
            else if (valid && !same) atomicAdd(&h[slot], 1u);
        }
    }
    __syncthreads();
    if (tid < DISPLAY_HIST_WORDS) scratch[(size_t)blockIdx.x * DISPLAY_HIST_WORDS + tid] = h[tid];
}

// Inclusive prefix sum over the 256 values that the threads tid < 256 hold (Hillis-Steele in LDS, 8 steps); EVERY thread of the block calls
// it (the barriers are the block's).  Returns the thread's prefix (0 for tid >= 256) and leaves the total in *total for every thread.
__device__ __forceinline__ uint32_t dp_scan256(uint32_t v, uint32_t (&buf)[2][256], uint32_t tid, uint32_t* total) {
    __syncthreads();                                              // the previous use of buf is over
    if (tid < 256u) buf[0][tid] = v;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (uint32_t off = 1u; off < 256u; off <<= 1) {
        if (tid < 256u) {
            uint32_t x = buf[cur][tid];
            if (tid >= off) x += buf[cur][tid - off];
            buf[cur ^ 1][tid] = x;
        }
        __syncthreads();
        cur ^= 1;
    }
    *total = buf[cur][255];
    return tid < 256u ? buf[cur][tid] : 0u;
}

// The second launch, one block.  Everything is integer until the last step, so the order of the additions is free: the rows are summed by four
// groups of 256 threads (independent loads, eight in flight per thread), the two trims are taken from prefix sums — bin k keeps
// min(n_k, max(P_k - cut, 0)) of what an ascending pass leaves, P the inclusive prefix sum; the descending pass likewise from the suffix sums
// of what is left — which is what the header's sequential rule gives; N' and S are LDS integer adds.  One thread does the float steps.
// prev may be record itself: that thread reads the one before it writes the other, and neither is __restrict__.
__global__ __launch_bounds__(DISPLAY_FINISH_BLOCK) void display_finish_kernel(const uint32_t* __restrict__ scratch, uint32_t rows, DisplayMeterArgs a, const uint32_t* prev,
                                                                             uint32_t* record, uint32_t* hist) {
    constexpr uint32_t GROUPS = DISPLAY_FINISH_BLOCK / 256u, EXTRA = DISPLAY_HIST_WORDS - 256u;
    static_assert(GROUPS == 4 && DISPLAY_METER_MAX_ROWS * EXTRA <= DISPLAY_FINISH_BLOCK, "one thread per row and extra column below");
    __shared__ uint32_t part[GROUPS][256];
    __shared__ uint32_t buf[2][256];
    __shared__ uint32_t edge[EXTRA];                               // below, above
    __shared__ unsigned long long red[2];                          // N', S
    const uint32_t tid = threadIdx.x, g = tid >> 8, c = tid & 255u;
    if (tid < EXTRA) edge[tid] = 0u;
    if (tid < 2u) red[tid] = 0ull;
    uint32_t s0 = 0u, r = g;                                       // column c over the rows g, g + 4, ...
    for (; r + 7u * GROUPS < rows; r += 8u * GROUPS) {
        uint32_t v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) v[j] = scratch[(size_t)(r + j * GROUPS) * DISPLAY_HIST_WORDS + c];
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) s0 += v[j];
    }
    for (; r < rows; r += GROUPS) s0 += scratch[(size_t)r * DISPLAY_HIST_WORDS + c];
    part[g][c] = s0;
    __syncthreads();
    // the two extra columns: thread t takes row t / 2, column 256 + t % 2 (rows <= 256: one load at most)
    if ((tid >> 1) < rows) atomicAdd(&edge[tid & 1u], scratch[(size_t)(tid >> 1) * DISPLAY_HIST_WORDS + 256u + (tid & 1u)]);
    uint32_t n = 0u;
    if (tid < 256u) {
        n = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        if (hist) hist[tid] = n;                                   // the histogram before the trims
    }
    uint32_t N = 0u, T1 = 0u;
    const uint32_t P = dp_scan256(n, buf, tid, &N);
    if (hist && tid < EXTRA) hist[256u + tid] = edge[tid];         // (dp_scan256's barriers are behind the adds)
    const uint64_t cut_lo = ((uint64_t)N * a.trim_low) >> 10, cut_hi = ((uint64_t)N * a.trim_high) >> 10;
    const uint32_t n1 = (uint64_t)P > cut_lo ? (uint32_t)min((uint64_t)n, (uint64_t)P - cut_lo) : 0u;
    const uint32_t P1 = dp_scan256(n1, buf, tid, &T1);
    const uint64_t Q = (uint64_t)T1 - P1 + n1;                     // the suffix sum of n1 at this bin
    const uint32_t n2 = Q > cut_hi ? (uint32_t)min((uint64_t)n1, Q - cut_hi) : 0u;
    if (tid < 256u && n2 != 0u) {
        atomicAdd(&red[0], (unsigned long long)n2);
        atomicAdd(&red[1], (unsigned long long)n2 * tid);
    }
    __syncthreads();
    if (tid != 0u) return;

    const uint64_t Np = red[0], S = red[1];
    const bool has_prev = prev != nullptr;
    const float e_prev = has_prev ? __uint_as_float(prev[0]) : 1.0f;
    float L = 0.0f, Et = e_prev;
    if (Np > 0) {
        const uint64_t pos = (S << 20) / Np;
        L = __uint_as_float((a.base << 20) + (uint32_t)pos + (1u << 19));
        const float q = a.key / L;
        Et = fminf(fmaxf(q, a.e_min), a.e_max);
    }
    float E = Et;
    if (has_prev && a.adapt != 1.0f) {
        const float d = Et - e_prev;
        const float m = d * a.adapt;
        E = e_prev + m;
    }
    record[0] = __float_as_uint(E); record[1] = __float_as_uint(Et); record[2] = __float_as_uint(L);
    record[3] = N; record[4] = edge[0]; record[5] = edge[1]; record[6] = (uint32_t)Np; record[7] = 0u;
}

template <int TONE, bool SRGB>
__global__ __launch_bounds__(256) void display_kernel(const float* __restrict__ film, uint64_t pixels, DisplayArgs a, const uint32_t* __restrict__ record,
                                                      float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float E = record ? __uint_as_float(record[0]) : a.exposure;
    const float* f = film + 3 * i;
    float x[3], v[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) x[ch] = fminf(dn_clean(f[ch], a.spp) * E, DP_X_MAX);
    if constexpr (TONE == MI355PT_TONE_REINHARD_EXT) {
        const float Y = dp_lum(x[0], x[1], x[2]);
        const float wa = Y / a.white2;
        const float wb = 1.0f + wa;
        const float n = Y * wb, d = 1.0f + Y;
        const float Yp = n / d;
        const float s = Yp / Y;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[ch] = Y == 0.0f ? 0.0f : x[ch] * s;
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (TONE == MI355PT_TONE_NONE) v[ch] = fminf(x[ch], 1.0f);
            else if constexpr (TONE == MI355PT_TONE_REINHARD) v[ch] = x[ch] / (1.0f + x[ch]);
            else if constexpr (TONE == MI355PT_TONE_ACES) v[ch] = dp_aces(x[ch]);
            else v[ch] = dp_hable(x[ch]) / a.hable_white;
        }
    }
    float* o = out + 3 * i;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch] = SRGB ? srgb_oetf(v[ch]) : v[ch];
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_display.cpp, which has checked every argument) ----
float display_hable(float x) { return dp_hable(x); }

hipError_t launch_display_hist(const float* d_film, const DisplayMeterArgs& args, uint32_t* d_scratch, hipStream_t stream) {
    const DisplayMeterPlan plan = plan_display_meter(args.width, args.height);
    if (plan.rows == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(display_hist_kernel, dim3(plan.rows), dim3(DISPLAY_METER_BLOCK), 0, stream, d_film, plan.pixels, plan.rows, plan.trips, args.spp, args.base,
                       d_scratch);
    return hipGetLastError();
}

hipError_t launch_display_finish(const uint32_t* d_scratch, const DisplayMeterArgs& args, const uint32_t* d_prev_record, uint32_t* d_record, uint32_t* d_hist,
                                 hipStream_t stream) {
    const DisplayMeterPlan plan = plan_display_meter(args.width, args.height);
    if (plan.rows == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(display_finish_kernel, dim3(1), dim3(DISPLAY_FINISH_BLOCK), 0, stream, d_scratch, plan.rows, args, d_prev_record, d_record, d_hist);
    return hipGetLastError();
}

hipError_t launch_display_meter(const float* d_film, const DisplayMeterArgs& args, const uint32_t* d_prev_record, uint32_t* d_scratch, uint32_t* d_record,
                                uint32_t* d_hist, hipStream_t stream) {
    const hipError_t e = launch_display_hist(d_film, args, d_scratch, stream);
    return e != hipSuccess ? e : launch_display_finish(d_scratch, args, d_prev_record, d_record, d_hist, stream);
}

hipError_t launch_display(const float* d_film, const DisplayArgs& args, const uint32_t* d_record, float* d_out, hipStream_t stream) {
    const DisplayMeterPlan plan = plan_display_meter(args.width, args.height);      // (the same frame limits: fewer than 2^32 pixels, so at most 2^24 blocks)
    if (plan.pixels == 0) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((plan.pixels + 255u) / 256u)), block(256);
#define PT_DP_LAUNCH(TONE, SRGB) hipLaunchKernelGGL((display_kernel<TONE, SRGB>), grid, block, 0, stream, d_film, plan.pixels, args, d_record, d_out)
#define PT_DP_TONE(TONE)                                                   \
    case TONE:                                                             \
        if (args.encode == MI355PT_ENCODE_SRGB) PT_DP_LAUNCH(TONE, true);  \
        else PT_DP_LAUNCH(TONE, false);                                    \
        break;
    switch (args.tone) {
        PT_DP_TONE(MI355PT_TONE_NONE)
        PT_DP_TONE(MI355PT_TONE_REINHARD)
        PT_DP_TONE(MI355PT_TONE_REINHARD_EXT)
        PT_DP_TONE(MI355PT_TONE_ACES)
        PT_DP_TONE(MI355PT_TONE_HABLE)
        default: return hipErrorInvalidValue;      // a missing kernel is an error, never another curve
    }
#undef PT_DP_TONE
#undef PT_DP_LAUNCH
    return hipGetLastError();
}

}  // namespace pt
