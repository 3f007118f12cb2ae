// The sample-loop kernel over an EXPLICIT TILE LIST (mi355pt_render_accum_tiles_device, the adaptive driver): pt_kernel's body text
// (pt_kernel_body.inc) under a second kernel name, with tile = tile_list(prm)[tile_k] where pt_kernel computes shard_index + tile_k *
// shard_count.  Everything else is pt_kernel's: work items, Sobol prefix tables, the LDS film tile, accum += tile, the chunk slots (laid
// out by POSITION in the list, like a shard's).  A second name rather than a template parameter of pt_kernel: the existing instantiations
// keep their mangled names and their device code (tools/asm_identity.sh).  No instrumented variant and no per-sample log.
// The instantiations live in pt_kernels_tiles*.hip, one unit per MODE and feature-set class with that class's backend options (Makefile);
// the feature sets, their two classes and the choice among them are pt_kernel's (launch_plan.hpp select_kernel), so a list of all tiles runs
// the very arithmetic of the plain launch.
#pragma once
#include "pt_kernel.hpp"

namespace pt {

// lane_job for a listed tile.  An index at or beyond the frame's tile count is clamped to the tile count, i.e. to tile row tiles_y: its
// py >= height, so it selects no pixel and writes nothing (the host refuses such a list, and the adaptive step never emits one).
PT_DEV LaneJob lane_job_tiles(uint32_t work, uint32_t lane, const DevCamera& cam, const DevParams& prm) {
    return lane_job_at(work, lane, cam, prm, [&](uint32_t tile_k) { return min(tile_list(prm)[tile_k], prm.tiles_x * prm.tiles_y); });
}

template <uint32_t FEAT, uint32_t MODE>
__global__ __launch_bounds__(64, kernel_min_waves<FEAT>()) void pt_kernel_tiles(DevScene sc, DevCamera cam, DevParams prm_in, const uint64_t* __restrict__ dim_hash_tab,
                                                float* __restrict__ accum, float* __restrict__ partial, unsigned* __restrict__ work_counter,
                                                DevStats* __restrict__ stats, PathOut pout, float4* __restrict__ defer_buf) {
    constexpr bool STATS = false;
#define PT_LANE_JOB lane_job_tiles
#include "pt_kernel_body.inc"
#undef PT_LANE_JOB
}

}  // namespace pt

// a tile-list unit's whole text, like PT_KERNELS_PLAIN / PT_KERNELS_CC (pt_kernel.hpp)
#define PT_KERNEL_TILES_CASE(F) case (F): return pt_kernel_tiles<(F), MODE>;
#define PT_KERNELS_TILES_PLAIN(M) PT_PRODUCTION_KERNELS(true, M, false, PT_FOR_EACH_PLAIN_SET, PT_KERNEL_TILES_CASE)
#define PT_KERNELS_TILES_CC(M) PT_PRODUCTION_KERNELS(true, M, true, PT_FOR_EACH_CC_SET, PT_KERNEL_TILES_CASE)
