// The sample-loop kernel over an EXPLICIT TILE LIST (mi355pt_render_accum_tiles_device, the adaptive driver): pt_kernel's body text
// (pt_kernel_body.inc) under a second kernel name, with tile = tile_list(prm)[tile_k] where pt_kernel computes shard_index + tile_k *
// shard_count.  Everything else is pt_kernel's: work items, Sobol prefix tables, the LDS film tile, accum += tile, the chunk slots (laid
// out by POSITION in the list, like a shard's).  A second name rather than a template parameter of pt_kernel: the existing instantiations
// keep their mangled names and their device code (tools/asm_identity.sh).  No instrumented variant and no per-sample log.
// The instantiations live in pt_kernels_tiles*.hip, one unit per MODE and feature-set class with that class's backend options (Makefile).
#pragma once
#include "pt_kernel.hpp"

namespace pt {

// lane_job for a listed tile.  An index at or beyond the frame's tile count is clamped to the tile count, i.e. to tile row tiles_y: its
// py >= height, so it selects no pixel and writes nothing (the host refuses such a list, and the adaptive step never emits one).
PT_DEV LaneJob lane_job_tiles(uint32_t work, uint32_t lane, const DevCamera& cam, const DevParams& prm) {
    LaneJob j{0, 0, 0, 0, false};
    const uint32_t b = prm.block_log2, bside = 1u << b;
    uint32_t item = work / prm.chunks, chunk = work % prm.chunks;
    uint32_t tile_k = item >> (6u - 2u * b), blk = item & ((64u >> (2u * b)) - 1u);
    uint32_t tile = min(tile_list(prm)[tile_k], prm.tiles_x * prm.tiles_y);
    uint32_t tx = tile % prm.tiles_x, ty = tile / prm.tiles_x;
    uint32_t bx = blk & ((8u >> b) - 1u), by = blk >> (3u - b);
    j.px = tx * 8 + bx * bside + (lane & (bside - 1u)); j.py = ty * 8 + by * bside + ((lane >> b) & (bside - 1u));
    j.valid = lane < (1u << (2u * b)) && j.px < cam.width && j.py < cam.height;
    j.s_cur = prm.sample_begin + chunk * prm.chunk_size;
    j.s_end = min(j.s_cur + prm.chunk_size, prm.sample_end);
    return j;
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

// ---- launch of the tile-list variants of one MODE: the feature sets, their two classes and the choice among them are pt_kernel's
// (pick_features, PT_FOR_EACH_PLAIN_SET / PT_FOR_EACH_CC_SET), so a list of all tiles runs the very arithmetic of the plain launch ----
#define PT_TILES_CASE(F) case (F): hipLaunchKernelGGL((pt_kernel_tiles<(F), MODE>), dim3(a.grid), dim3(64), 0, a.stream, a.sc, a.cam, a.prm, a.d_hash, a.d_accum, a.d_partial, a.d_counter, a.d_stats, a.pout, a.d_defer); break;
template <uint32_t MODE>
void launch_pt_tiles_plain(const PtLaunchArgs& a, uint32_t feat) {
    switch (pick_features(feat)) { PT_FOR_EACH_PLAIN_SET(PT_TILES_CASE) default: break; }
}
template <uint32_t MODE>
void launch_pt_tiles_cc(const PtLaunchArgs& a, uint32_t feat) {
    switch (pick_features(feat)) { PT_FOR_EACH_CC_SET(PT_TILES_CASE) default: break; }
}
#undef PT_TILES_CASE
void launch_pt_tiles_mis_sobol(const PtLaunchArgs& a, uint32_t feat);      // pt_kernels_tiles_mis.hip (plain sets; forwards the clearcoat sets)
void launch_pt_tiles_mis_sobol_cc(const PtLaunchArgs& a, uint32_t feat);   // pt_kernels_tiles_mis_cc.hip
void launch_pt_tiles_nee_sobol(const PtLaunchArgs& a, uint32_t feat);      // pt_kernels_tiles_nee.hip
void launch_pt_tiles_nee_sobol_cc(const PtLaunchArgs& a, uint32_t feat);   // pt_kernels_tiles_nee_cc.hip
void launch_pt_tiles_strategy_pt(const PtLaunchArgs& a, uint32_t feat);    // pt_kernels_tiles_pt.hip

}  // namespace pt
