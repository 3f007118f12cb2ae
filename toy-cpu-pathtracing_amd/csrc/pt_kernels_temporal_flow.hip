// The flow-aware twins of the temporal accumulation and of the rectified form's gather (include/mi355pt_flow.h): the body of
// pt_kernels_temporal.hip and pt_kernels_temporal_rectify.hip (pt_temporal_gather.inc) with PT_TP_MOTION == 2 — the pixel's own 32-byte
// motion record, two coalesced 16-byte loads, is added to the hit position and to the normal — and those units' two epilogues.  A unit of
// its own: the two existing units keep their text and their device code.  EXTENSION, no reference counterpart.  One thread per pixel,
// 64 x 4 blocks, no LDS, no atomics, no scratch memory.  Launched with a previous frame only (HAS_PREV == true): the first frame
// reprojects nothing and takes temporal_accumulate_kernel.  The rectified form's second launch is the rectify unit's blend, like every carry's.
//
// Every operation is a single binary32 operation in the order the headers state (the unit is built with -ffp-contract=off and calls no
// fmaf), divisions are IEEE: the result is bit-equal to tests/flow_reference.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.hpp"
#include "pt_denoise_common.hpp"
#include "pt_temporal_gather.hpp"

namespace pt {

namespace {

template <bool HAS_HALF, bool HAS_PREV, bool HAS_PREV_IDS>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_accumulate_flow_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a, FlowArgs fl,
                                                                                           float* __restrict__ out_film, float* __restrict__ out_half,
                                                                                           float* __restrict__ out_length) {
#define PT_TP_RECORD false
#define PT_TP_MOTION 2
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

template <bool HAS_HALF, bool HAS_PREV, bool HAS_PREV_IDS>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_gather_flow_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a, FlowArgs fl,
                                                                                       float4* __restrict__ record) {
#define PT_TP_RECORD true
#define PT_TP_MOTION 2
#include "pt_temporal_gather.inc"
#undef PT_TP_MOTION
#undef PT_TP_RECORD

    tp_write_record(record, p, m1, m2, L);
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_temporal.cpp's driver, which has checked every argument) ----
hipError_t launch_temporal_accumulate_flow(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const FlowArgs& flow, float* d_out_film,
                                           float* d_out_half, float* d_out_length, hipStream_t stream) {
    const TpShape sh = tp_shape(args);
    tp_dispatch(cur.half != nullptr, flow.ids_prev != nullptr, [&](auto half, auto ids) {
        hipLaunchKernelGGL((temporal_accumulate_flow_kernel<decltype(half)::value, true, decltype(ids)::value>), sh.grid, sh.block, 0, stream, cur, prev, args, flow,
                           d_out_film, d_out_half, d_out_length);
    });
    return hipGetLastError();
}

hipError_t launch_temporal_gather_flow(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const FlowArgs& flow, void* d_scratch,
                                       hipStream_t stream) {
    const TpShape sh = tp_shape(args);
    tp_dispatch(cur.half != nullptr, flow.ids_prev != nullptr, [&](auto half, auto ids) {
        hipLaunchKernelGGL((temporal_gather_flow_kernel<decltype(half)::value, true, decltype(ids)::value>), sh.grid, sh.block, 0, stream, cur, prev, args, flow,
                           (float4*)d_scratch);
    });
    return hipGetLastError();
}

}  // namespace pt
