// The flow-aware twins of the temporal accumulation and of the rectified form's gather (include/mi355pt_flow.h): the body of
// pt_kernels_temporal.hip and pt_kernels_temporal_rectify.hip (pt_temporal_gather.inc) with PT_TP_MOTION == 2 — the pixel's own 32-byte
// motion record, two coalesced 16-byte loads, is added to the hit position and to the normal — and those units' two epilogues.  A unit of
// its own: the two existing units keep their text and their device code.  EXTENSION, no reference counterpart.  One thread per pixel,
// 64 x 4 blocks, no LDS, no atomics, no scratch memory.  Launched with a previous frame only (HAS_PREV == true): the first frame
// reprojects nothing and takes temporal_accumulate_kernel.  The rectified form's second launch is the rectify unit's own blend.
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

static_assert(TEMPORAL_RECTIFY_RECORD_BYTES == 2 * sizeof(float4), "a scratch record is two float4");

template <bool HAS_HALF, bool HAS_PREV, bool HAS_PREV_IDS>
__global__ __launch_bounds__(DN_BLOCK_X * DN_BLOCK_Y) void temporal_gather_flow_kernel(TemporalFrameDev cur, TemporalFrameDev prev, TemporalArgs a, FlowArgs fl,
                                                                                       float4* __restrict__ record) {
#define PT_TP_RECORD true
#define PT_TP_MOTION 2
#include "pt_temporal_gather.inc"
#undef PT_TP_MOTION
#undef PT_TP_RECORD

    record[2 * p] = make_float4(m1[0], m1[1], m1[2], m2[0]);
    record[2 * p + 1] = make_float4(m2[1], m2[2], L, 0.0f);
}

}  // namespace

// ---- host side (declared in launch.hpp; called from api_flow.cpp, which has checked every argument) ----
hipError_t launch_temporal_accumulate_flow(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const FlowArgs& flow, float* d_out_film,
                                           float* d_out_half, float* d_out_length, hipStream_t stream) {
    args.blocks_x = (uint32_t)(((uint64_t)args.width + DN_BLOCK_X - 1) / DN_BLOCK_X);
    const dim3 grid(denoise_grid_blocks(args.width, args.height)), block(DN_BLOCK_X, DN_BLOCK_Y);
    const bool has_half = cur.half != nullptr, has_ids = flow.ids_prev != nullptr;
#define PT_TP_LAUNCH(HALF, IDS) \
    hipLaunchKernelGGL((temporal_accumulate_flow_kernel<HALF, true, IDS>), grid, block, 0, stream, cur, prev, args, flow, d_out_film, d_out_half, d_out_length)
    if (has_half && has_ids) PT_TP_LAUNCH(true, true);
    else if (has_half) PT_TP_LAUNCH(true, false);
    else if (has_ids) PT_TP_LAUNCH(false, true);
    else PT_TP_LAUNCH(false, false);
#undef PT_TP_LAUNCH
    return hipGetLastError();
}

hipError_t launch_temporal_rectify_flow(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const FlowArgs& flow, uint32_t radius,
                                        float gamma, void* d_scratch, float* d_out_film, float* d_out_half, float* d_out_length, hipStream_t stream) {
    if (radius < 1 || radius > 3) return hipErrorInvalidValue;
    args.blocks_x = (uint32_t)(((uint64_t)args.width + DN_BLOCK_X - 1) / DN_BLOCK_X);
    const dim3 grid(denoise_grid_blocks(args.width, args.height)), block(DN_BLOCK_X, DN_BLOCK_Y);
    float4* record = (float4*)d_scratch;
    const bool has_half = cur.half != nullptr, has_ids = flow.ids_prev != nullptr;
#define PT_TR_GATHER(HALF, IDS) hipLaunchKernelGGL((temporal_gather_flow_kernel<HALF, true, IDS>), grid, block, 0, stream, cur, prev, args, flow, record)
    if (has_half && has_ids) PT_TR_GATHER(true, true);
    else if (has_half) PT_TR_GATHER(true, false);
    else if (has_ids) PT_TR_GATHER(false, true);
    else PT_TR_GATHER(false, false);
#undef PT_TR_GATHER
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_temporal_rectify_blend(cur, args, radius, gamma, d_scratch, d_out_film, d_out_half, d_out_length, stream);
}

}  // namespace pt
