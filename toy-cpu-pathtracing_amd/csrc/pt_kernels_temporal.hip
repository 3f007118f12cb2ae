// The temporal reprojection of include/mi355pt_temporal.h — the temporal half of SVGF (Schied et al., HPG 2017) beside the spatial filter
// of pt_kernels_denoise_var.hip — as one plain HIP gather kernel for gfx950.  EXTENSION, no reference counterpart.  It keeps the denoisers'
// shape: one thread per pixel, 64 x 4 blocks, no LDS, no atomics, no scratch.
//
// The kernel's body is pt_temporal_gather.inc (the gather, which pt_kernels_temporal_rectify.hip runs too) with the blend as its epilogue;
// that file says how the taps are loaded and why.
//
// Every operation is a single binary32 operation in the order the header states (the unit is built with -ffp-contract=off and calls no
// fmaf), divisions are IEEE: the result is bit-equal to tests/temporal_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

// SLOTS film values per channel travel through the blend: (c1, c2) with a half film, (c) without
template <bool HAS_HALF, bool HAS_PREV>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_accumulate_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a,
                                                                                      float* __restrict__ out_film, float* __restrict__ out_half,
                                                                                      float* __restrict__ out_length) {
#define PT_TP_RECORD false
#define PT_TP_MOTION false
#include "pt_temporal_gather.inc"
#undef PT_TP_MOTION
#undef PT_TP_RECORD

    out_length[p] = L;
    if constexpr (HAS_HALF) {
        out_half[3 * p] = m1[0]; out_half[3 * p + 1] = m1[1]; out_half[3 * p + 2] = m1[2];
        out_film[3 * p] = m1[0] + m2[0]; out_film[3 * p + 1] = m1[1] + m2[1]; out_film[3 * p + 2] = m1[2] + m2[2];
    } else {
        out_film[3 * p] = m1[0]; out_film[3 * p + 1] = m1[1]; out_film[3 * p + 2] = m1[2];
    }
}

// The motion-aware twin (include/mi355pt_motion.h): the same body with PT_TP_MOTION, the same epilogue.  Launched with a previous frame
// only (HAS_PREV == true): the first frame reprojects nothing and takes the kernel above
template <bool HAS_HALF, bool HAS_PREV, bool HAS_PREV_IDS>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_accumulate_motion_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a,
                                                                                             MotionArgs mo, float* __restrict__ out_film,
                                                                                             float* __restrict__ out_half, float* __restrict__ out_length) {
#define PT_TP_RECORD false
#define PT_TP_MOTION true
#include "pt_temporal_gather.inc"
#undef PT_TP_MOTION
#undef PT_TP_RECORD

    out_length[p] = L;
    if constexpr (HAS_HALF) {
        out_half[3 * p] = m1[0]; out_half[3 * p + 1] = m1[1]; out_half[3 * p + 2] = m1[2];
        out_film[3 * p] = m1[0] + m2[0]; out_film[3 * p + 1] = m1[1] + m2[1]; out_film[3 * p + 2] = m1[2] + m2[2];
    } else {
        out_film[3 * p] = m1[0]; out_film[3 * p + 1] = m1[1]; out_film[3 * p + 2] = m1[2];
    }
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_temporal.cpp's driver, which has checked every argument) ----
hipError_t launch_temporal_accumulate(const TemporalFrameDev& cur, const TemporalFrameDev* prev, TemporalArgs args, float* d_out_film, float* d_out_half,
                                      float* d_out_length, hipStream_t stream) {
    const TpShape sh = tp_shape(args);
    const TemporalFrameDev pv = prev ? *prev : TemporalFrameDev{};
    tp_dispatch(cur.half != nullptr, prev != nullptr, [&](auto half, auto has_prev) {
        hipLaunchKernelGGL((temporal_accumulate_kernel<decltype(half)::value, decltype(has_prev)::value>), sh.grid, sh.block, 0, stream, cur, pv, args, d_out_film,
                           d_out_half, d_out_length);
    });
    return hipGetLastError();
}

hipError_t launch_temporal_accumulate_motion(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const MotionArgs& motion,
                                             float* d_out_film, float* d_out_half, float* d_out_length, hipStream_t stream) {
    const TpShape sh = tp_shape(args);
    tp_dispatch(cur.half != nullptr, motion.ids_prev != nullptr, [&](auto half, auto ids) {
        hipLaunchKernelGGL((temporal_accumulate_motion_kernel<decltype(half)::value, true, decltype(ids)::value>), sh.grid, sh.block, 0, stream, cur, prev, args,
                           motion, d_out_film, d_out_half, d_out_length);
    });
    return hipGetLastError();
}

}  // namespace pt
