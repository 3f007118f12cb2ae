// The sample-loop kernel template (see pt_kernels.hip for the design notes).  A header so that the specialisations by MODE and feature-set
// class are compiled in separate translation units, in parallel and with their own backend options (Makefile): pt_kernels.hip (generic +
// instrumented), pt_kernels_mis[_cc].hip, pt_kernels_nee[_cc].hip, pt_kernels_pt.hip.  Each unit is a PT_KERNELS_PLAIN / PT_KERNELS_CC line per class it
// holds (below) and nothing else; which instantiation a launch takes is decided once, in launch_plan.hpp select_kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "launch_plan.hpp"
#include "layout.hpp"
#include "pt_device.hpp"
#include "pt_path.hpp"
#include "tail_queue_plan.hpp"
// (a wave-uniform value the compiler cannot see as one — it came through LDS — goes back to a scalar register)
#define PT_CAM_UNIFORM(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#include "camera_candidates.hpp"

namespace pt {

// CAMERA RAYS FROM A LIST (camera_candidates.hpp): the kernels with the tail queue find, once per work item, the triangles a camera ray of
// the item's pixel block can hit (a walk of the 4-wide tree against the block's pyramid of directions, by the whole wave in lockstep) and
// keep up to CAM_LIST_CAP indices in LDS.  A fresh camera ray then takes its hit from that list — the ring flush's own triangle test on each
// candidate, the atomicMin merge's own key, winner_hit — and stays out of the cooperative traversal; an iteration that holds only fresh
// camera rays skips the traversal.  A list that overflows, DevScene::cam_lists == 0 (launch_plan.hpp use_camera_lists), and every other
// kernel: the traversal for every ray, as before.  cam_n == CAM_LIST_NONE says so.
constexpr uint32_t CAM_LIST_NONE = 0xffffffffu;

#ifndef PT_MIN_WAVES_CC
#define PT_MIN_WAVES_CC 3
#endif
#ifndef PT_MIN_WAVES
#define PT_MIN_WAVES 4   // 128 VGPRs: measured +26 % over the unconstrained 220-VGPR build (latency hiding beats the spills)
#endif
// work item -> lane assignment
struct LaneJob { uint32_t px, py, s_cur, s_end; bool valid; };
// tile_of(tile_k): the frame tile of the launch's tile_k-th tile (lane_job: of the shard; pt_kernel_tiles.hpp lane_job_tiles: of the list)
template <typename TileOf>
PT_DEV LaneJob lane_job_at(uint32_t work, uint32_t lane, const DevCamera& cam, const DevParams& prm, TileOf tile_of) {
    LaneJob j{0, 0, 0, 0, false};
    // work = ((tile * blocks per tile) + block) * chunks + chunk; lanes >= 4^b own no pixel of the block
    const uint32_t b = prm.block_log2, bside = 1u << b;
    uint32_t item = work / prm.chunks, chunk = work % prm.chunks;
    uint32_t tile_k = item >> (6u - 2u * b), blk = item & ((64u >> (2u * b)) - 1u);
    uint32_t tile = tile_of(tile_k);
    uint32_t tx = tile % prm.tiles_x, ty = tile / prm.tiles_x;
    uint32_t bx = blk & ((8u >> b) - 1u), by = blk >> (3u - b);
    j.px = tx * 8 + bx * bside + (lane & (bside - 1u)); j.py = ty * 8 + by * bside + ((lane >> b) & (bside - 1u));
    j.valid = lane < (1u << (2u * b)) && j.px < cam.width && j.py < cam.height;
    j.s_cur = prm.sample_begin + chunk * prm.chunk_size;
    j.s_end = min(j.s_cur + prm.chunk_size, prm.sample_end);
    return j;
}
PT_DEV LaneJob lane_job(uint32_t work, uint32_t lane, const DevCamera& cam, const DevParams& prm) {
    return lane_job_at(work, lane, cam, prm, [&](uint32_t tile_k) { return prm.shard_index + tile_k * prm.shard_count; });
}

PT_DEV void flush_stats(DevStats* stats, const StatCounters& st) {
    atomicAdd(&stats->samples, (unsigned long long)st.samples);
    atomicAdd(&stats->closest_rays, (unsigned long long)st.closest_rays);
    atomicAdd(&stats->shadow_rays, (unsigned long long)st.shadow_rays);
    atomicAdd(&stats->nodes_closest, (unsigned long long)st.nodes_closest);
    atomicAdd(&stats->tris_closest, (unsigned long long)st.tris_closest);
    atomicAdd(&stats->nodes_shadow, (unsigned long long)st.nodes_shadow);
    atomicAdd(&stats->tris_shadow, (unsigned long long)st.tris_shadow);
    atomicAdd(&stats->closest_hits, (unsigned long long)st.closest_hits);
    atomicAdd(&stats->bounces, (unsigned long long)st.bounces);
    atomicAdd(&stats->spectrum_evals, (unsigned long long)st.spectrum_evals);
    atomicAdd(&stats->textured_lookups, (unsigned long long)st.textured_lookups);
    for (int i = 0; i < 8; ++i) if (st.w[i]) atomicAdd(&stats->wave_steps[i], (unsigned long long)st.w[i]);
    for (int i = 0; i < 16; ++i) if (st.hist[i]) atomicAdd(&stats->busy_hist[i >> 3][i & 7], (unsigned long long)st.hist[i]);
    for (int i = 0; i < 4; ++i) if (st.dv[i]) atomicAdd(&stats->divergence[i], (unsigned long long)st.dv[i]);
    if (st.ties) atomicAdd(&stats->phase_cycles[9], (unsigned long long)st.ties | ((unsigned long long)st.ties_differ << 32));
}

// Wave priority by stage (s_setprio; the SIMD's issue arbitration goes by priority, then age): a wave in a traversal is a chain of dependent
// round trips and loses nothing by yielding the issue port, a wave in the shading stage has independent work to issue — shading and hand-out
// run at priority 3, traversals at 0.  Measured: +0.9...+1.3 % (scenes 3 / 0 / 8 / 17; 0.0 on 15 / 19); the other way round -1.1 %.
#define PT_PRIO_TRAV_ENTER __builtin_amdgcn_s_setprio(0)
#define PT_PRIO_TRAV_EXIT __builtin_amdgcn_s_setprio(3)
// ONE cooperative traversal per iteration for the next closest-hit rays AND the light connections of the vertex just shaded (trace_pair_coop,
// pt_device.hpp): a wave's step count is bounded by its deepest ray, not by the ray count, so the two traversals together cost ~20 node
// steps instead of ~18 + ~14.  The price is the pending connection's 11 registers across one more stage, and a heavier loop where there
// are no connections at all.  Measured per kernel (same box):
//   kernels without the clearcoat code: +2.4...+5 % (scene 3 1 716 -> 1 757, scene 0 1 814 -> 1 906, scene 8 1 525 -> 1 574, scene 10 1 519 -> 1 583);
//   clearcoat kernels (3 waves per SIMD), with the LDS parking and the sinking in place: MIS +1.7 / +5.5 % (scenes 15 / 19); NEE +2.2 % (scene 17,
//   C5's kernel: 1 242 -> 1 270), +2.2 / +3.6 % (scenes 16 / 20), +1.5 % (scene 19) — but -1.1 / -2.1 % in the clearcoat + texture set under NEE or
//   the generic mode (scenes 15 / 18), which keeps two traversals;
//   the plain path tracer (strategy pt: no connections exist) loses 9 % with it (scene 3 2 790 vs 2 557): it has its own specialisation
//   (MODE_PT, pt_kernels_pt.hip) without it; choosing inside one kernel at run time costs both sides (-5 % / -8 %: measured);
//   generic-mode clearcoat kernels (random sampler with NEE / MIS): not measured, two traversals as before.
// (MODE_*: launch_plan.hpp)
// (the *_of functions: the same statements on values, for the launcher's queue size, queue_bytes_per_wave below)
constexpr bool merged_traversal_of(uint32_t FEAT, uint32_t MODE) {
    if (MODE == MODE_PT) return false;
    if ((FEAT & FEAT_CC) == 0u || MODE == MODE_MIS_SOBOL) return true;
    return MODE == MODE_NEE_SOBOL && FEAT != (FEAT_CC | FEAT_TEX);
}
template <uint32_t FEAT, uint32_t MODE> constexpr bool merged_traversal() { return merged_traversal_of(FEAT, MODE); }
// MATERIAL SORT BETWEEN BOUNCES, wave-local (the deferral queue; defer_classes() below says which kernels have it).  A wave shades all
// its lanes together, so an iteration in which a few lanes hit the hero pays the hero's whole BSDF branch on top of the room's: measured 19-52 k of ~270-300 k cycles per iteration wherever the scene
// has a second material class, i.e. in 84-93 % of the iterations for 8-13 % of the lanes.  With the queue a lane whose closest
// hit lies on a DEFERRED class (the clearcoat material in the kernels that have it, the dielectrics in theirs) does not shade: it writes its
// path and the hit to the wave's own queue in global memory (128 B per path, a ring of 128 entries per resident wave; L2-resident) and is
// FREE — it starts a new camera path at the top of the next iteration like a lane whose path ended, so no lane idles for the sort.  When at
// least PT_DEFER_MIN paths wait (or the work item has no new paths left), the lanes that are free after the shading stage take queued paths
// and the wave shades them at once in a second pass: the minority branch runs once for ~30 lanes instead of in every iteration for ~6
// (measured +11...+34 %, dielectrics +-0; taking the queued paths at the top of the iteration instead, where they sit out its traversal:
// +4 % scene 17, -5...-9 % dielectrics).  A path only ever waits in the queue of the wave that owns its pixel's LDS film tile, the order of pushes and pops is a function of the wave's own
// deterministic schedule, and a sample's arithmetic does not depend on when it is shaded: frames stay bit-identical from run to run and
// sample-for-sample equal to the oracle's.  (Moving paths BETWEEN waves — the usual wavefront formulation — needs 9 KB of LDS per queue or
// float atomics on the film; sorting inside the wave's own time line needs neither.)
#ifndef PT_DEFER_MIN
#define PT_DEFER_MIN 56         // paths waiting before the queue is shaded (20 / 28 / 40 / 48 / 60 measured: scene 17 1 497 / 1 512 / 1 523 / 1 528 / 1 529)
#endif
constexpr uint32_t DEFER_RING = 128u;           // entries per wave: a drain starts at PT_DEFER_MIN waiting paths and one iteration adds at most 64
constexpr uint32_t DEFER_F4 = 8u;               // float4 per entry
constexpr uint32_t defer_classes_of(uint32_t FEAT, uint32_t MODE) {    // bit c: sort class c (MT_* | 8 if the material has a spectrum texture, DevTri::pad[0]) is deferred
    if (!merged_traversal_of(FEAT, MODE)) return 0u;
    // the clearcoat material wherever it exists (its branch is the longest: +12 % scene 17, +22 % scene 19, +34 % scene 15); in the kernels
    // without it, the materials with a spectrum texture (bilinear fetches + rgb2spec cells; C2's hero: +0.6 %, scene 4 +0.8 %; a class for
    // every textured material lost 4 % on the normal-map-only hero of scene 5).  The dielectrics alone measured +-0 (their branch is short)
    // and are not deferred.
    if ((FEAT & FEAT_CC) != 0u) return (1u << MT_CLEARCOAT) | (1u << (MT_CLEARCOAT | 8u));
    if ((FEAT & FEAT_TEX) != 0u) return 0xff00u;
    return 0u;
}
template <uint32_t FEAT, uint32_t MODE> constexpr uint32_t defer_classes() { return defer_classes_of(FEAT, MODE); }
// TAIL QUEUE (PT_TAILQ): the same idea for EVERY path.  A third of the lanes that enter the shading stage end their path in its front
// (emission, roulette) and used to idle through BSDF sampling and the light connection — 28 % of a wave's time at 65 % of its lanes.  Now the
// shading stage is two: (1) the FRONT of the vertex for every lane that traced (emission with its weight, throughput, roulette, depth:
// shade_vertex_head<PHASE 1>); the paths that go on are written to the wave's queue (path + hit) and ALL lanes are free; (2) when 64 paths wait, one pass takes them into the free lanes and runs the back of the vertex (the surface again from
// the hit, frames, the BSDF's draws: <PHASE 2>) and the tail — BSDF sample, light connection — for a FULL wave.  Lanes left free start new
// camera paths as before.  In the clearcoat kernels the paths whose hit is on the clearcoat material have a queue of their own, so a pass
// shades one class (this subsumes the deferral queue there); when a work item has nothing new left, whatever waits shares the passes.  A sample's
// arithmetic and its sampler dimensions are what they were — the record carries the path between the two halves of ITS vertex —, the
// queues belong to the wave that owns the pixels, the schedule is the wave's own: frames bit-identical from run to run, 166 GPU tests
// unchanged.  Same-box A/B (round 3): **C2 2 088 -> 2 312 Msamples/s (+10.7 %), C3 +11.9 %, C4 +13.2 %, C5 1 574 -> 1 893 (+20 %)**, scene 19
// +37 %, scene 15 +22 %, scenes 0 / 5 +10 / +12 %.  Measured on the way: a threshold of 48 instead of 64 waiting paths gives +7 % instead of
// +10.7 % (passes not full); a second queue for every class but plain Lambert in the kernels WITHOUT clearcoat loses everything again
// (a class that is a tenth of the hits leaves up to 63 paths to be bounced out in sparse passes at the end of every work item); writing
// the pass with the back of the head and the tail in two divergent regions instead of one costs those kernels 12 % (ShadeCtx across a
// re-convergence point at 128 VGPRs, as round 1 found for the fused shader).
// Each queue is a STACK (tail_queue_plan.hpp has the index arithmetic, tests/test_tail_queue_plan.py runs it on the CPU): a pass pops the
// NEWEST records.  Popped first in, first out — the queues were rings once — a pass read the OLDEST records, written one or two iterations
// earlier, and the head walked round every slot of every wave's queue: 512 waves x 10 KB per XCD against a 4 MB L2, every record a miss in
// both directions.  Newest first, most of a pass's records are the ones the front has just stored, and the bottom of the
// stack goes cold until the work item drains.  The order of the pops is still a function of the wave's own state, so frames stay
// bit-identical from run to run; a pixel's samples reach the LDS film tile in another order than with the rings, so the film's float sums
// differ from that build's in the last bits (per-sample values do not: tests/test_tail_queue_order_gpu.py).
// STAGING (the kernels with ONE queue; tail_queue_plan.hpp tq_stage_*, tests/test_tail_queue_stage.py): when the push of an iteration
// makes a pass due, that pass — in the same iteration, every lane being free — pops the newest min(64, count) records, and those include
// all of the <= 64 just pushed.  Such records need no memory: the front writes them to LDS, into the traversal stack (s_stack: used only
// inside trace_*, holding nothing between two traversals; 64 records x 80 B = 5 KB of its 6 KB, so no new LDS), in the global stack's
// own field-major layout over 64 slots, and the pass reads them back from there.  Logically they still lie on top of the stack: the pass
// hands each free lane the slot tq_pop_slot names, a slot at or above the pre-push count comes from LDS, one below it from the global
// stack, and the count ends where it would — the record -> lane mapping, the order in which a pixel's samples reach the film tile and so
// the film are bit for bit those of the all-global path (tests/test_tail_queue_stage_gpu.py).  In C2's cadence (three pushes of ~43 after
// a pass, one of ~62 camera paths, a pass at 64) three pushes in four are followed by a pass: 148 of 191 records never leave the CU.  A
// push without a pass goes to the global stack as before.  The two-queue kernels do not stage: their class-2-first rule lets a pass leave
// fresh records of the other class behind.  MI355PT_NO_QUEUE_STAGING=1 (launch_plan.hpp, DevScene::queue_stage) sends every record through
// the global stack again: the A/B control (profiles/queue_stage_ab.json).
#ifndef PT_TAILQ
#define PT_TAILQ 1
#endif
#ifndef PT_TAILQ_MIN
#define PT_TAILQ_MIN 64
#endif
constexpr bool tail_queue_of(uint32_t FEAT, uint32_t MODE) { return PT_TAILQ != 0 && merged_traversal_of(FEAT, MODE); }    // (the clearcoat kernels too: two queues, one per sort class)
template <uint32_t FEAT, uint32_t MODE> constexpr bool tail_queue() { return tail_queue_of(FEAT, MODE); }
constexpr uint32_t QUEUE_RING = (PT_TAILQ != 0) ? 256u : DEFER_RING;     // entries per wave and queue (the capacity of a stack of the two-queue kernels; of the deferral ring)
constexpr uint32_t QUEUE_MAX = (PT_TAILQ != 0) ? 2u : 1u;               // queues per wave (the tail queue keeps one per sort class)
// (the queue's records are written once and read once, but stores / loads with the non-temporal hint, meant to keep them from pushing the
// BVH out of the L2 — L2 hit rate 0.98 before the queues, 0.89 with them — measured -4 % (C2 2 578 -> 2 481, C4 -5.6 %): the records then
// come back from HBM instead of the L2 / Infinity Cache)
static_assert(PT_TAILQ == 0 || QUEUE_RING == 256u, "the tail queue's entry index keeps the queue number in bit 8");
constexpr uint32_t TQ_F4 = 5u;                                           // float4 per record of the tail queue (80 B; the deferral queue's record: DEFER_F4)
// entries of the stack where one queue suffices: at most 127 paths ever wait there (tail_queue_plan.hpp), and the smaller stack keeps the
// records closer to the L2
#ifndef PT_TAILQ_RING1
#define PT_TAILQ_RING1 128u
#endif
// LIGHT-HIT QUEUE (the kernels with ONE tail queue; tail_queue_plan.hpp lq_*, tests/test_light_queue.py).  The last minority branch of the
// front: a BSDF-sampled ray of the Cornell room reaches the ceiling light with a probability of 1 to 2 %, so in a good third of the
// iterations one or two lanes of 64 ran the whole emitter evaluation (pt_path.hpp emitter_hit: surface, material and spectrum records — three
// dependent loads —, the radiance, the MIS weight) while the wave waited.  A path that arrives at an emitter ends there.  So the front
// pushes it — L, T, the spawning sample's f and pdf, the vertex left, the ray direction, the hit, the wavelengths, the pixel: 7 float4 =
// 112 B, field-major on a stack of LQ_SLOTS entries behind the tail queue's in the wave's region of the queue buffer — and the lane is
// free: no throughput update, no roulette draw for a path that ends regardless.  When 64 wait, one pass right after the front (every lane
// is free, no path state is live) calls emitter_hit for a full wave and finishes the 64 samples to the film; when the work item is done
// one last pass takes what is left.  A sample's arithmetic is what it was — per-sample values are bit for bit those of the in-place
// path, tests/test_light_queue_gpu.py —, the schedule is the wave's own: frames bit-identical from run to run; a pixel's samples reach the
// film tile in another order, as when the queues became stacks.  MI355PT_NO_LIGHT_QUEUE=1 (launch_plan.hpp, DevScene::light_queue)
// evaluates in place again: the A/B control (profiles/light_queue_ab.json).
constexpr uint32_t LQ_F4 = 7u;                                           // float4 per record of the light-hit queue (112 B)
constexpr bool light_queue_of(uint32_t FEAT, uint32_t MODE) { return tail_queue_of(FEAT, MODE) && (FEAT & FEAT_CC) == 0u; }
// Queue memory of one resident wave of pt_kernel<STATS, FEAT, MODE> / pt_kernel_tiles<FEAT, MODE> (STATS = false), in bytes: what that
// kernel's queues hold and nothing more — 24 KB for one stack and the light-hit queue ((5 + 7) float4 x 128 entries), 40 KB for the clearcoat kernels' two (2 x 5 x 256),
// 16 KB for the instrumented kernels' deferral ring, 0 for a kernel without a queue.  The ONE statement of the per-wave stride: the kernel
// body places its queues with it (q_base) and the launcher sizes the buffer with it for the kernel it selected (query_defer_bytes_per_wave).
constexpr size_t queue_bytes_per_wave(bool STATS, uint32_t FEAT, uint32_t MODE) {
    if (!STATS && tail_queue_of(FEAT, MODE)) return (size_t)16u * TQ_F4 * ((FEAT & FEAT_CC) != 0u ? QUEUE_MAX * QUEUE_RING : PT_TAILQ_RING1) + (light_queue_of(FEAT, MODE) ? (size_t)16u * LQ_F4 * LQ_SLOTS : (size_t)0);
    return defer_classes_of(FEAT, MODE) != 0u ? (size_t)16u * DEFER_F4 * DEFER_RING : (size_t)0;
}
// MODE compiles the renderer strategy and the sampler in (MODE_GENERIC reads them from DevParams): the branches on
// prm.strategy / the sampler mode fold away, worth +2.5 % on C2 (MIS + Sobol), +1.3 % on C5 (NEE + Sobol).
// The cooperative traversals walk the 4-wide tree (both trees are on the device; the plain traversals of the probes and of the canonical-count
// mode walk the BVH2).  Measured: it halves the dependent node round trips per ray (18 -> ~10 wave steps per closest-hit trace): +3...4.5 %
// on every kernel, and +4.7 % on the kernel specialised for textured Lambert scenes (C2's) once that kernel stopped spilling around the wider
// step (round 2: machine LICM off, see the Makefile; before that the same tree cost it 4 % and it kept the BVH2).
// Waves per SIMD of the clearcoat kernels.  Round 2: 3 (168 VGPRs) with the spawning sample's record parked in LDS.  Since the material sort
// moved most clearcoat shading into dedicated passes, the common iteration is the room's: the kernels whose clearcoat code is not
// ALSO carrying the texture code gain from a fourth wave (128 VGPRs, no parking: the LDS is needed for 16 waves) — scene 17 NEE (C5) +1.8 %,
// scene 19 (all-features kernel) +3.6 %, scenes 16 / 17 MIS +0 ... 0.5 %; the clearcoat + texture set loses 5.8 % (scene 15: 276 B of scratch) and stays at 3.
template <uint32_t FEAT> constexpr int kernel_min_waves() {
    if ((FEAT & FEAT_CC) == 0u) return PT_MIN_WAVES;
    if (FEAT != (FEAT_CC | FEAT_TEX)) return 4;
    return PT_MIN_WAVES_CC;
}
template <bool STATS, uint32_t FEAT, uint32_t MODE = MODE_GENERIC>
__global__ __launch_bounds__(64, kernel_min_waves<FEAT>()) void pt_kernel(DevScene sc, DevCamera cam, DevParams prm_in, const uint64_t* __restrict__ dim_hash_tab,
                                                float* __restrict__ accum, float* __restrict__ partial, unsigned* __restrict__ work_counter,
                                                DevStats* __restrict__ stats, PathOut pout, float4* __restrict__ defer_buf) {
#define PT_LANE_JOB lane_job
#include "pt_kernel_body.inc"
#undef PT_LANE_JOB
}

// ---- the Sobol prefix tables of pt_kernel's work loop as a function, for the AOV kernel (pt_kernels_aov.hip), which takes the same work
// items and draws with the same sampler code.  pt_kernel keeps its own inline spelling of the same statements: calling this function
// from it changes the instruction schedule of every tuned path kernel (compared on the gfx950 disassembly), and those are measured as
// they are.  A change to one side belongs on the other as well. ----
// Block-uniform Sobol digit prefixes of a work item (pt_device.hpp sampler_index), where the launch shape allows them: lane d computes
// dimensions d, d + 64, ... < n_dims for this block (job0: lane 0's job, whose pixel is the block origin) into s_hi / s_p6 and sctx is
// pointed at them.  Single-pixel items over an aligned 4^m block of sample indices: the sample digits above m are part of the prefix.
// The caller synchronises before the first draw.  (n_dims may be smaller than SOBOL_HI_DIMS only together with tables of SOBOL_HI_DIMS
// entries or in a kernel that never draws a dimension from n_dims on: sampler_index reads the tables for every dimension below SOBOL_HI_DIMS.)
PT_DEV void item_sobol_prefixes(SamplerCtx& sctx, const DevParams& prm, const LaneJob& job0, uint32_t lane, uint32_t* s_hi, uint32_t* s_p6, uint32_t n_dims) {
    const uint32_t blk_log2 = prm.block_log2;
    const uint32_t s_prefix = prm.sample_prefix_digits;
    // (the tables hold the permuted prefix in 27 bits per entry: a launch shape whose prefix is wider hashes every digit instead)
    const uint32_t hi_first_w = sobol_hi_first(prm.log2_spp, blk_log2) - s_prefix, hi_shift_w = 2u * hi_first_w - (prm.log2_spp & 1u);
    if (prm.sampler == 1u && hi_first_w < prm.n_base4_digits && hi_first_w >= 3u &&
        2u * prm.n_base4_digits - (prm.log2_spp & 1u) <= hi_shift_w + 27u) {
        sctx.hi_first = sobol_hi_first(prm.log2_spp, blk_log2) - s_prefix;
        sctx.hi_shift = 2u * sctx.hi_first - (prm.log2_spp & 1u);
        const uint32_t tile_m = (encode_morton2_u32(job0.px, job0.py) << prm.log2_spp) | (s_prefix ? job0.s_cur : 0u);
        for (uint32_t dmn = lane; dmn < n_dims; dmn += 64) {
            uint32_t e = (uint32_t)(sobol_tile_hi_digits(tile_m, dmn, prm.log2_spp, prm.n_base4_digits, sctx.hi_first) >> sctx.hi_shift);   // <= 26 bits: the Morton index is a u32 and hi_shift >= 6
            const uint64_t prefix = (uint64_t)tile_m >> sctx.hi_shift;                 // the digits above digit hi_first-1
            e |= sobol_perm_index(prefix, dmn) << 27;
            uint32_t e6 = 0;
            for (uint32_t v7 = 0; v7 < 4u; ++v7) e6 |= sobol_perm_index((prefix << 2) | v7, dmn) << (5u * v7);
            s_hi[dmn] = e; s_p6[dmn] = e6;
        }
        sctx.hi_lds = s_hi; sctx.p6_lds = s_p6;
    }
}
// ---- the instantiations, by address ----
// pt_kernel and pt_kernel_tiles (pt_kernel_tiles.hpp) share their parameter list: one pointer type for every path kernel.
using PtKernel = void (*)(DevScene, DevCamera, DevParams, const uint64_t*, float*, float*, unsigned*, DevStats*, PathOut, float4*);
// The production instantiation of the feature set `set` among those of one (plain or tile-list kernel, MODE, feature-set class); nullptr:
// not a set of that class.  Each is specialised — and its kernels with it instantiated — in exactly one translation unit, whose whole text
// is the line PT_KERNELS_PLAIN(mode) or PT_KERNELS_CC(mode) (pt_kernel_tiles.hpp: PT_KERNELS_TILES_*).  pt_kernels.hip's find_pt_kernel is
// the lookup over all of them: launch and occupancy query take the pointer from there.
template <bool TILES, uint32_t MODE, bool CC> PtKernel production_kernel(uint32_t set);
#define PT_PRODUCTION_KERNELS(TILES, MODE_, CC, FOR_EACH_SET, CASE)                       \
    namespace pt {                                                                        \
    template <> PtKernel production_kernel<TILES, MODE_, CC>(uint32_t set) {              \
        constexpr uint32_t MODE = MODE_;                                                  \
        switch (set) { FOR_EACH_SET(CASE) default: return nullptr; }                      \
    }                                                                                     \
    }
#define PT_KERNEL_CASE(F) case (F): return pt_kernel<false, (F), MODE>;
#define PT_KERNELS_PLAIN(M) PT_PRODUCTION_KERNELS(false, M, false, PT_FOR_EACH_PLAIN_SET, PT_KERNEL_CASE)
#define PT_KERNELS_CC(M) PT_PRODUCTION_KERNELS(false, M, true, PT_FOR_EACH_CC_SET, PT_KERNEL_CASE)

}  // namespace pt
