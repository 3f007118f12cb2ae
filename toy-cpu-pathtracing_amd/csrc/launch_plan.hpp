// The shape of a launch as a pure function of (camera, params, sample range, resident waves): the tiles of the shard, the pixel block and
// sample chunk of a work item, the Sobol prefix digits, the grid.  Host only — integer arithmetic on the C ABI's structs and layout.hpp's,
// no HIP — so that tests/test_launch_plan.py checks what the kernels' lane_job and prefix-table code rely on without a GPU.
// And WHICH path kernel the launch takes (select_kernel, at the end), as pure: the one statement of that choice, tests/test_kernel_select.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355pt.h"
#include "layout.hpp"

namespace pt {

struct V3 { float x, y, z; };
inline V3 cross3(V3 a, V3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline V3 norm3(V3 a) { float r = 1.0f / std::sqrt((a.x * a.x) + (a.y * a.y) + (a.z * a.z)); return {a.x * r, a.y * r, a.z * r}; }

inline uint32_t log2_int(uint32_t v) { return v == 0 ? 0 : 31 - (uint32_t)__builtin_clz(v); }
inline uint32_t round_up_pow2(uint32_t v) { return v <= 1 ? 1 : 1u << (32 - __builtin_clz(v - 1)); }

// 8x8 tiles of a width x height frame that belong to a shard: tiles shard_index, shard_index + shard_count, ... (shard_count 0 = whole frame)
inline uint32_t shard_tile_count(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count) {
    const uint32_t total = ((width + 7) / 8) * ((height + 7) / 8);
    const uint32_t cnt = shard_count ? shard_count : 1u, idx = shard_count ? shard_index : 0u;
    return total > idx ? (total - idx + cnt - 1) / cnt : 0u;
}

inline DevCamera make_camera(const mi355pt_camera* c) {
    DevCamera d{};
    V3 f = norm3(V3{c->direction[0], c->direction[1], c->direction[2]});       // set_look_to normalises (camera.rs:46-48)
    V3 up = norm3(V3{c->up[0], c->up[1], c->up[2]});
    V3 s = norm3(cross3(f, up));                                                // glam Mat3::look_to_rh
    V3 u = cross3(s, f);
    d.s[0] = s.x; d.s[1] = s.y; d.s[2] = s.z; d.u[0] = u.x; d.u[1] = u.y; d.u[2] = u.z; d.f[0] = f.x; d.f[1] = f.y; d.f[2] = f.z;
    float fov_rad = c->fov_deg * (3.14159265358979323846f / 180.0f);
    d.tan_half_fov = std::tan(fov_rad / 2.0f);
    d.aspect = (float)c->width / (float)c->height;
    d.width = c->width; d.height = c->height;
    return d;
}

// GamutSrgb::new().xyz_to_rgb() (color/src/gamut.rs:29-63), glam Mat3 arithmetic in f32
inline void srgb_xyz_to_rgb(float out_rowmajor[9]) {
    auto xy = [](float x, float y) { return V3{x * 1.0f / y, 1.0f, (1.0f - x - y) * 1.0f / y}; };
    V3 r = xy(0.64f, 0.33f), g = xy(0.30f, 0.60f), b = xy(0.15f, 0.06f), w = xy(0.3127f, 0.3290f);
    auto inv = [](V3 x, V3 y, V3 z, V3 o[3]) {   // returns columns of the inverse
        V3 t0 = cross3(y, z), t1 = cross3(z, x), t2 = cross3(x, y);
        float det = (z.x * t2.x) + (z.y * t2.y) + (z.z * t2.z);
        float id = 1.0f / det;
        V3 r0{t0.x * id, t0.y * id, t0.z * id}, r1{t1.x * id, t1.y * id, t1.z * id}, r2{t2.x * id, t2.y * id, t2.z * id};
        o[0] = V3{r0.x, r1.x, r2.x}; o[1] = V3{r0.y, r1.y, r2.y}; o[2] = V3{r0.z, r1.z, r2.z};
    };
    auto mulv = [](const V3 m[3], V3 v) {
        return V3{m[0].x * v.x + m[1].x * v.y + m[2].x * v.z, m[0].y * v.x + m[1].y * v.y + m[2].y * v.z, m[0].z * v.x + m[1].z * v.y + m[2].z * v.z};
    };
    V3 rgb[3] = {r, g, b}, irgb[3];
    inv(r, g, b, irgb);
    V3 c = mulv(irgb, w);
    V3 r2x[3] = {V3{rgb[0].x * c.x, rgb[0].y * c.x, rgb[0].z * c.x}, V3{rgb[1].x * c.y, rgb[1].y * c.y, rgb[1].z * c.y},
                 V3{rgb[2].x * c.z, rgb[2].y * c.z, rgb[2].z * c.z}};
    V3 x2r[3];
    inv(r2x[0], r2x[1], r2x[2], x2r);
    // row-major: row i = (col0[i], col1[i], col2[i])
    out_rowmajor[0] = x2r[0].x; out_rowmajor[1] = x2r[1].x; out_rowmajor[2] = x2r[2].x;
    out_rowmajor[3] = x2r[0].y; out_rowmajor[4] = x2r[1].y; out_rowmajor[5] = x2r[2].y;
    out_rowmajor[6] = x2r[0].z; out_rowmajor[7] = x2r[1].z; out_rowmajor[8] = x2r[2].z;
}

inline DevParams make_params(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end) {
    DevParams d{};
    d.spp = p->spp; d.seed = p->seed; d.max_depth = p->max_depth; d.strategy = p->strategy; d.sampler = p->sampler;
    d.exposure = p->exposure;
    d.rr_gate = 1.0f - p->rr_gate_slack;
    d.albedo_lut = p->albedo_lut ? 1u : 0u;
    d.log2_spp = log2_int(p->spp);                                              // ZSobolSampler::new (:179-196)
    uint32_t res = round_up_pow2(std::max(cam->width, cam->height));
    d.n_base4_digits = log2_int(res) + (d.log2_spp + 1) / 2;
    d.sample_begin = s_begin; d.sample_end = s_end;
    d.shard_count = p->shard_count ? p->shard_count : 1;
    d.shard_index = p->shard_count ? p->shard_index : 0;
    d.tiles_x = (cam->width + 7) / 8; d.tiles_y = (cam->height + 7) / 8;
    srgb_xyz_to_rgb(d.xyz_to_rgb);
    return d;
}

constexpr uint32_t PT_MAX_LAUNCH_SAMPLES = 4096;
// The launches of a sample range: launch(begin, end) -> int (0 = go on) for each, in order; returns the first non-zero result.
// `timed`: the caller wants the stats of ONE launch, so the range is not broken up.
template <typename Launch>
int for_each_launch_range(uint32_t sampler, bool timed, uint32_t s_begin, uint32_t s_end, Launch&& launch) {
    if (sampler == MI355PT_SAMPLER_SOBOL && !timed && s_end - s_begin > PT_MAX_LAUNCH_SAMPLES) {
        // long Sobol ranges go out as aligned blocks of 4096 sample indices: single-pixel work items over an aligned 4^6 block hash the
        // fewest digits per draw (the digits above the block join the prefix tables), and no launch runs for minutes
        for (uint32_t b = s_begin; b < s_end;) {
            const uint32_t e = std::min(s_end, (b / PT_MAX_LAUNCH_SAMPLES + 1u) * PT_MAX_LAUNCH_SAMPLES);
            if (int rc = launch(b, e)) return rc;
            b = e;
        }
        return 0;
    }
    return launch(s_begin, s_end);
}

struct LaunchPlan {
    DevParams params;        // complete but for stats_mode (the launcher's)
    uint32_t n_tiles;        // 8x8 tiles of the shard (0: nothing to launch)
    int grid;                // one-wave workgroups
    size_t partial_floats;   // per-chunk film tiles of a split launch (0: chunks == 1)
};

// One launch over the sample indices [s_begin, s_end) on a device that holds `waves` resident waves of the kernel.
// aov: the AOV kernel (pt_kernels_aov.hip) — the same work items, but never a split sample range
// n_tiles: the 8x8 tiles the launch covers (plan_launch: the shard's; plan_launch_tiles: the entries of a list) — the shape depends on their
// NUMBER only
inline LaunchPlan plan_launch_over(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, int waves, bool aov, uint32_t n_tiles) {
    DevParams dp = make_params(cam, p, s_begin, s_end);
    if (aov) { dp.exposure = 1.0f; dp.rr_gate = 1.0f; dp.strategy = 0u; dp.max_depth = 0u; dp.albedo_lut = 0u; }   // Sensor::new(spp, 1.0, NoneToneMap), albedo_renderer.rs:43-44
    // Work items.  A work item is a 2^b x 2^b pixel block of an 8x8 tile times a range of sample indices, its (pixel, sample)
    // pairs handed to the lanes as a pool.  Sobol: the fewer pixels an item has, the fewer Morton digits vary inside it, and only
    // varying digits (minus the two that have block-level tables) are hashed per draw (pt_device.hpp sampler_index): take the
    // smallest block that still gives the pool >= PT_MIN_ITEM_SAMPLES pairs, so lanes keep finding new paths and the
    // per-item prefix tables stay amortised.
    uint32_t n_samples = s_end - s_begin;
    uint32_t block_log2 = 3;
    uint64_t PT_MIN_ITEM_SAMPLES = 2048;
#ifdef MI355PT_TUNING   // launch-shape sweeps (tools/block_sweep.sh, chunk_sweep.sh): not in the shipped library
    if (const char* e = getenv("MI355PT_MIN_ITEM")) PT_MIN_ITEM_SAMPLES = (uint64_t)std::max(64, atoi(e));
#endif
    if (dp.sampler == MI355PT_SAMPLER_SOBOL) {
        while (block_log2 > 0 && ((uint64_t)n_samples << (2u * (block_log2 - 1u))) >= PT_MIN_ITEM_SAMPLES) --block_log2;
    }
#ifdef MI355PT_TUNING
    if (const char* e = getenv("MI355PT_BLOCK")) { int b = atoi(e); if (b >= 0 && b <= 3) block_log2 = (uint32_t)b; }
#endif
    // the permuted block-uniform digits (everything above bit hi_shift of the 2 n - odd bit sample index) are packed into 27 bits
    // of a table word: large frames (>= 16384 pixels wide) need a larger block
    {
        const uint32_t odd = dp.log2_spp & 1u, index_bits = 2u * dp.n_base4_digits - odd;
        auto hi_shift = [&](uint32_t b) { return 2u * ((dp.log2_spp + 1u) / 2u + b) - odd; };
        while (block_log2 < 3 && (hi_shift(block_log2) < 6u || index_bits > hi_shift(block_log2) + 27u)) ++block_log2;
    }
    dp.block_log2 = block_log2;
    const uint32_t n_items = n_tiles * (64u >> (2u * block_log2));
    // split the sample range only when there are too few items to fill the chip (small images / many shards): about 8 work
    // items per resident wave, but no chunk under 16 samples (every work item rebuilds its Sobol prefix tables; measured
    // with tools/chunk_sweep.sh: one shard of 4 / 8 at 1080p is 2.2 % / 0.9 % faster with 16-sample than with 8-sample chunks)
    // (while some resident waves would have no item at all, chunks may go down to 8 samples: a 256x256 frame has 1 024 tiles)
    // (the AOV kernel never splits: its tiles continue the film's sums in sample order, so that consecutive sample ranges compose bit for bit)
    uint32_t chunks = 1;
    while (!aov && n_items * chunks < (uint32_t)waves * 8 && chunks * 2 <= n_samples &&
           (n_samples / (chunks * 2)) >= (n_items * chunks >= (uint32_t)waves ? 16u : 8u)) chunks *= 2;
#ifdef MI355PT_TUNING
    if (const char* e = getenv("MI355PT_CHUNKS")) { uint32_t c = (uint32_t)atoi(e); if (c >= 1 && c <= n_samples) chunks = c; }
#endif
    dp.chunks = chunks; dp.chunk_size = (n_samples + chunks - 1) / chunks;
    dp.n_work = n_items * chunks;
    // single-pixel items whose sample ranges are aligned blocks of 4^m indices: the sample digits above m are item-uniform as well
    dp.sample_prefix_digits = 0;
    if (dp.sampler == MI355PT_SAMPLER_SOBOL && block_log2 == 0 && (dp.log2_spp & 1u) == 0u && n_samples % chunks == 0) {
        const uint32_t cs = dp.chunk_size;
        uint32_t m = 0;
        while ((1u << (2u * (m + 1u))) <= cs) ++m;
        if ((1u << (2u * m)) == cs && s_begin % cs == 0 && m >= 3 && m <= dp.log2_spp / 2u &&
            2u * dp.n_base4_digits <= 2u * m + 27u) dp.sample_prefix_digits = dp.log2_spp / 2u - m;   // prefix above bit 2m must fit 27 bits
    }
    const int grid = (int)std::min<uint32_t>(dp.n_work, (uint32_t)waves);
    // one slot per 8x8 tile and chunk, whatever the block size
    return LaunchPlan{dp, n_tiles, grid, dp.chunks > 1 ? (size_t)n_tiles * dp.chunks * 64u * 3u : (size_t)0};
}
inline LaunchPlan plan_launch(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, int waves, bool aov) {
    return plan_launch_over(cam, p, s_begin, s_end, waves, aov, shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count));
}
// One launch of the tile-list kernels (pt_kernel_tiles.hpp) over n_list tiles of the whole frame (p->shard_count 0 or 1): tile_k counts the
// list's entries, so the shape is that of a shard with n_list tiles — and, for n_list = every tile of the frame, field for field
// plan_launch's whole-frame plan: a list of all tiles renders today's frame bit for bit.  The launcher puts the list's device address into
// params (layout.hpp set_tile_list) in place of the shard pair.
inline LaunchPlan plan_launch_tiles(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, int waves, uint32_t n_list) {
    return plan_launch_over(cam, p, s_begin, s_end, waves, false, n_list);
}

// ---- which path kernel a launch takes (tests/test_kernel_select.py) ----
// MODE compiles the renderer strategy and the sampler into the kernel (pt_kernel.hpp); MODE_GENERIC reads them from DevParams.
enum : uint32_t { MODE_GENERIC = 0, MODE_MIS_SOBOL = 1, MODE_NEE_SOBOL = 2, MODE_PT = 3, MODE_COUNT = 4 };
// The compiled feature sets, ONE ordered list in two classes: P(set) for the sets without the clearcoat code, then C(set) for those with it.
// The classes are compiled in separate translation units with their own backend options (Makefile): the plain sets run at 4 waves per SIMD
// and gain from sinking / the AMDGPU pressure trackers, the clearcoat sets (3 waves per SIMD) lose.  A scene runs the FIRST set of the list
// that covers its features (pick_features), so within a class a set stands before every set that contains it.
#define PT_FOR_EACH_SET(P, C)                                                                                                          \
    P(0u) P(FEAT_TEX) P(FEAT_DIEL) P(FEAT_METAL) P(FEAT_DIEL | FEAT_ROUGH) P(FEAT_DELTA | FEAT_MLIGHT) P(FEAT_STD & ~FEAT_CC)           \
    C(FEAT_CC) C(FEAT_CC | FEAT_TEX) C(FEAT_STD) C(FEAT_ALL)
#define PT_NO_SET(F)
#define PT_FOR_EACH_PLAIN_SET(X) PT_FOR_EACH_SET(X, PT_NO_SET)
#define PT_FOR_EACH_CC_SET(X) PT_FOR_EACH_SET(PT_NO_SET, X)
#define PT_SET_ENTRY(F) (F),
inline constexpr uint32_t FEATURE_SETS[] = {PT_FOR_EACH_SET(PT_SET_ENTRY, PT_SET_ENTRY)};
inline constexpr uint32_t PLAIN_SETS[] = {PT_FOR_EACH_PLAIN_SET(PT_SET_ENTRY)};
inline constexpr uint32_t CC_SETS[] = {PT_FOR_EACH_CC_SET(PT_SET_ENTRY)};
#undef PT_SET_ENTRY
// smallest compiled feature set covering `feat`
inline uint32_t pick_features(uint32_t feat) {
    for (uint32_t s : FEATURE_SETS) if ((feat & ~s) == 0u) return s;
    return FEAT_ALL;
}
// One kernel instantiation: pt_kernel_tiles<set, mode> (tiles), pt_kernel<stats, set, mode> otherwise.  The clearcoat class is set & FEAT_CC.
struct KernelKey { bool tiles, stats; uint32_t mode, set; };
// The kernel of a launch over the shard's tiles or over a tile list (tiles), with the instrumentation or without (stats), for a scene with
// the features `feat`.  The two instrumented variants are generic-mode kernels: scenes without the clearcoat code get the one whose traversal
// has the production form (merged, 4 waves per SIMD), so that the lane-use diagnostics describe what the benchmarked kernels do.  There is no
// instrumented tile-list kernel: the key says what was asked for, the lookup (pt_kernels.hip find_pt_kernel) finds nothing for it.
inline KernelKey select_kernel(bool tiles, bool stats, uint32_t feat, uint32_t sampler, uint32_t strategy) {
    if (stats) return KernelKey{tiles, true, MODE_GENERIC, (feat & (FEAT_CC | FEAT_EMTEX)) == 0u ? FEAT_STD & ~FEAT_CC : FEAT_ALL};
    const uint32_t mode = sampler == MI355PT_SAMPLER_SOBOL && strategy == MI355PT_STRATEGY_MIS ? MODE_MIS_SOBOL
                        : sampler == MI355PT_SAMPLER_SOBOL && strategy == MI355PT_STRATEGY_NEE ? MODE_NEE_SOBOL
                        : strategy == MI355PT_STRATEGY_PT ? MODE_PT : MODE_GENERIC;
    return KernelKey{tiles, false, mode, pick_features(feat)};
}

// ---- camera-ray candidate lists (camera_candidates.hpp, pt_kernel_body.inc) ----
// Does the launch take its camera-ray hits from per-work-item triangle lists (DevScene::cam_lists)?  Only the production kernels with the
// tail queue have the code (pt_kernel.hpp tail_queue_of: the instrumented kernels, the plain path tracer and the two-traversal clearcoat
// kernels walk the tree for every ray as before).  Every block size builds lists: measured, the 8x8 items of a 64-index launch gain 2.2 %
// with them (95 % of scene 3's 8x8 blocks stay within the cap) and lose 0.5 % without (profiles/camera_list_ab.json); block_log2 is the
// place to exclude a shape should one lose.  `enabled`: camera_lists_enabled().
inline bool use_camera_lists(const KernelKey& key, uint32_t block_log2, bool enabled) { return enabled && !key.stats && block_log2 <= 3u; }
// the host-side switch, read per launch: MI355PT_NO_CAMERA_LISTS=1 (any value but "0") turns the lists off; default on
inline bool camera_lists_enabled() { const char* e = getenv("MI355PT_NO_CAMERA_LISTS"); return !(e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0')); }

// ---- tail-queue staging (tail_queue_plan.hpp, pt_kernel_body.inc) ----
// Do the kernels with one tail queue keep the records a pass takes in the same iteration in LDS (DevScene::queue_stage)?  The kernels
// without the code (two queues, the instrumented ones, the plain path tracer) ignore the flag.  `enabled`: queue_staging_enabled().
inline bool use_queue_staging(const KernelKey& key, bool enabled) { return enabled && !key.stats; }
// the host-side switch, read per launch: MI355PT_NO_QUEUE_STAGING=1 (any value but "0") sends every record through the global stack; default on
inline bool queue_staging_enabled() { const char* e = getenv("MI355PT_NO_QUEUE_STAGING"); return !(e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0')); }

// ---- the light-hit queue (tail_queue_plan.hpp lq_*, pt_kernel_body.inc) ----
// Do the kernels with one tail queue push the paths that arrive at an emitter to the wave's light-hit queue (DevScene::light_queue)?  The
// kernels without the code (two queues, the instrumented ones, the plain path tracer) ignore the flag.  `enabled`: light_queue_enabled().
inline bool use_light_queue(const KernelKey& key, bool enabled) { return enabled && !key.stats; }
// the host-side switch, read per launch: MI355PT_NO_LIGHT_QUEUE=1 (any value but "0") evaluates every emitter hit in place; default on
inline bool light_queue_enabled() { const char* e = getenv("MI355PT_NO_LIGHT_QUEUE"); return !(e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0')); }

// ---- the early end of roulette-doomed paths (path_end_plan.hpp, pt_kernel_body.inc) ----
// Do the kernels with one tail queue end a doomed path without tracing its last ray when that ray cannot matter (DevScene::early_path_end)?
// With 0 they take the same decision in the same place — the roulette draw moved to the pass with it — and trace every ray: the control for
// the samples' values, not the speed of a build without the code.  The kernels without the code (two queues, the instrumented ones, the
// plain path tracer) ignore the flag.  `enabled`: early_path_end_enabled().
inline bool use_early_path_end(const KernelKey& key, bool enabled) { return enabled && !key.stats; }
// the host-side switch, read per launch: MI355PT_NO_EARLY_PATH_END=1 (any value but "0") traces every ray; default on
inline bool early_path_end_enabled() { const char* e = getenv("MI355PT_NO_EARLY_PATH_END"); return !(e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0')); }

}  // namespace pt
