// Every host-callable function a .hip translation unit defines for the host files (api.cpp, the api_*.cpp and scene_*.cpp files, through
// api_internal.hpp), declared ONCE: the callers and the defining
// units include this header, so a signature that drifts is a compile error (and PathOut, a kernel parameter, has one definition).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "launch_plan.hpp"
#include "layout.hpp"

namespace pt {

// Per-sample log (mi355pt_render_sample_log): when L != nullptr every finished path of the launch also writes its spectral radiance,
// wavelengths and wavelength pdfs to slot ((tile_k * 64 + pixel in tile) * n_s + (sample index - s_base)).  A wave-uniform branch at
// path end in the PRODUCTION kernel: the per-sample parity tests read what the benchmarked binary computed, in its own launch shape.
struct PathOut { float* L; float* lam; float* pdf; uint32_t s_base, n_s; };

// pt_kernels.hip: the path-tracing kernels, film resolve, multi-device gather, probes.
// launch_pt: the kernel `key` names (launch_plan.hpp select_kernel), wherever it is compiled, and the matching combine kernel when the sample
// range is split; hipErrorInvalidDeviceFunction when no such kernel is built.  n_tiles: the 8x8 tiles of the launch's shard (plan_launch) or,
// with key.tiles, the entries of the device list that prm carries (layout.hpp set_tile_list, plan_launch_tiles): the production kernels over
// an explicit tile list, which have no instrumented variant and write no sample log.
hipError_t launch_pt(const KernelKey& key, const DevScene&, const DevCamera&, const DevParams&, uint32_t n_tiles, const uint64_t* d_hash, float* d_accum,
                     float* d_partial, unsigned* d_counter, DevStats* d_stats, int grid, hipStream_t, const PathOut&, float* d_defer);
int query_resident_waves(const KernelKey& key);      // of the very kernel launch_pt takes for `key`
size_t query_defer_bytes_per_wave(const KernelKey& key);
hipError_t launch_resolve(const float* d_accum, uint32_t n_values, uint32_t spp, float* d_out, hipStream_t);
hipError_t launch_film_pack(const float* film, uint32_t w, uint32_t h, uint32_t shard_index, uint32_t shard_count, uint32_t n_tiles, float* packed, hipStream_t);
hipError_t launch_film_unpack(float* film, uint32_t w, uint32_t h, uint32_t shard_index, uint32_t shard_count, uint32_t n_tiles, const float* packed, hipStream_t);
hipError_t launch_probe_sobol(uint32_t width, uint32_t seed, uint32_t log2_spp, uint32_t nb4, const uint32_t* d_xys, uint32_t n, const uint8_t* d_pat,
                              uint32_t n_pat, uint32_t per, uint32_t* d_out, hipStream_t);
hipError_t launch_probe_intersect(const DevScene&, const float* o, const float* d, uint32_t n, float* t, uint32_t* inst, uint32_t* tri, float* nrm, hipStream_t);
hipError_t launch_probe_occluded(const DevScene&, const float* o, const float* d, const float* tmax, uint32_t n, uint8_t* out, hipStream_t);
hipError_t launch_probe_sincos(uint32_t first, uint32_t stride, uint32_t n, float* out_s, float* out_c, hipStream_t);
uint64_t host_murmur_dim_seed(uint32_t dimension, uint32_t seed);
// pt_kernels_aov.hip: the AOV renderers' primary-ray kernel (kind = MI355PT_AOV_*)
hipError_t launch_aov(uint32_t kind, const DevScene&, const DevCamera&, const DevParams&, uint32_t illuminant_lut, const uint64_t* d_hash, float* d_accum,
                      unsigned* d_counter, DevStats* d_stats, uint32_t feat, int grid, hipStream_t);
int query_resident_waves_aov(uint32_t kind, uint32_t feat);
hipError_t launch_aov_resolve(uint32_t kind, const float* d_accum, uint32_t n_values, uint32_t spp, float* d_out, hipStream_t);
// pt_kernels_gbuffer.hip: the G-buffer pass (include/mi355pt_gbuffer.h): one primary-ray launch, up to four films (nullptr = not wanted).
// The plan must have block_log2 == 3 and chunks == 1 (api_gbuffer.cpp plan_gbuffer): one pixel per lane, its sums in registers
struct GbufferFilms { float *albedo, *shading_normal, *position, *hit; };
hipError_t launch_gbuffer(const DevScene&, const DevCamera&, const DevParams&, uint32_t illuminant_lut, const uint64_t* d_hash, const GbufferFilms&,
                          unsigned* d_counter, DevStats* d_stats, uint32_t feat, int grid, hipStream_t);
int query_resident_waves_gbuffer(uint32_t feat);
hipError_t launch_gbuffer_normalize(const float* d_film, const float* d_hit, uint32_t n_pixels, float* d_out, hipStream_t);
// pt_kernels_denoise.hip: the a-trous denoiser (include/mi355pt_denoise.h)
size_t denoise_scratch_bytes(uint32_t width, uint32_t height);
uint32_t denoise_grid_blocks(uint32_t width, uint32_t height);
hipError_t launch_denoise(const float* d_beauty, uint32_t spp_b, const float* d_albedo, uint32_t spp_a, const float* d_normal, uint32_t spp_n,
                          uint32_t width, uint32_t height, uint32_t levels, float sigma_color, float sigma_normal, float sigma_albedo,
                          float albedo_eps, void* d_scratch, float* d_out, hipStream_t);
// pt_kernels_adaptive.hip: adaptive sampling's noise step and the per-tile normalisation (include/mi355pt_adaptive.h)
uint32_t adaptive_tile_count(uint32_t width, uint32_t height);      // 0: empty frame, or 2^31 tiles and more
size_t adaptive_scratch_bytes(uint32_t width, uint32_t height);
hipError_t launch_adaptive_step(const float* d_film, float* d_half, uint32_t width, uint32_t height, uint32_t* d_tile_spp, float* d_tile_err,
                                float threshold, float dark_eps, uint32_t level_spp, uint32_t max_spp, void* d_scratch, uint32_t* d_list,
                                uint32_t* d_count, hipStream_t);
hipError_t launch_normalize_tiles(const float* d_film, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_mean, hipStream_t);
// ... and the step's second launch alone: the ascending list of the tiles whose flag is not 0 and their number (pt_kernels_budget.hip's
// select pass is followed by it)
hipError_t launch_adaptive_compact(const uint32_t* d_flags, uint32_t n_tiles, uint32_t* d_list, uint32_t* d_count, hipStream_t);
// pt_kernels_denoise_var.hip: the variance-guided a-trous denoiser (include/mi355pt_denoise_var.h); its level launches take the grid of
// denoise_grid_blocks.  d_tile_spp == nullptr: every pixel has spp_b samples
size_t denoise_var_scratch_bytes(uint32_t width, uint32_t height);
hipError_t launch_denoise_var(const float* d_beauty, const float* d_half, uint32_t spp_b, const uint32_t* d_tile_spp, const float* d_albedo, uint32_t spp_a,
                              const float* d_normal, uint32_t spp_n, uint32_t width, uint32_t height, uint32_t levels, float sigma_lum, float sigma_normal,
                              float sigma_albedo, float albedo_eps, float lum_eps, void* d_scratch, float* d_out, hipStream_t);
// pt_kernels_temporal.hip, pt_kernels_temporal_rectify.hip: the temporal reprojection (include/mi355pt_temporal.h,
// mi355pt_temporal_rectify.h, mi355pt_motion.h, mi355pt_flow.h), every launch on the grid of denoise_grid_blocks; api_temporal.cpp's driver
// composes them.  A frame's films as the kernels take them (half == nullptr: no half film; length is read of the previous frame only).
// Every launcher fills its own copy of TemporalArgs::blocks_x
struct TemporalFrameDev { const float *film = nullptr, *half = nullptr, *length = nullptr, *position = nullptr, *shading_normal = nullptr, *hit = nullptr; };
struct TemporalArgs {
    uint32_t width, height, blocks_x;
    float spp, half_spp;                    // (float)spp, (float)(spp / 2)
    float wf, hf;                           // (float)width, (float)height
    float delta[3], rows[9], sx, sy, cx, cy;
    float pos_tol, normal_cos, min_weight, max_history;
};
// How a pixel's hit is carried into the previous frame beside the view: not at all (the static world, args.delta), through a per-instance
// table (a record as the kernels load it: six 16-byte loads, so the table is 16-byte aligned; last_entry = n_entries - 1, the clamp of a
// pixel's id) or through a 32-byte record per pixel (two 16-byte loads; ids_cur is read only with ids_prev).  ids_prev == nullptr: no id
// test of the taps.  With a table or records, args.delta is not read.  The kernels and the budget's probe take the same struct
struct MotionXformDev { float a[9], b[3], n[9], pad[3]; };
static_assert(sizeof(MotionXformDev) == 96, "a motion record is six float4");
struct FlowPixelDev { float d[3]; uint32_t id; float dn[3]; uint32_t pad; };
static_assert(sizeof(FlowPixelDev) == 32, "a flow record is two float4");
enum TemporalCarryKind : uint32_t { CARRY_STATIC = 0, CARRY_TABLE = 1, CARRY_FLOW = 2 };
struct TemporalCarryDev {
    const uint32_t *ids_cur = nullptr, *ids_prev = nullptr;
    const MotionXformDev* table = nullptr; uint32_t last_entry = 0;
    TemporalCarryKind kind = CARRY_STATIC;
    const FlowPixelDev* flow = nullptr;
};
struct TemporalOutsDev { float *film = nullptr, *half = nullptr, *length = nullptr; };
// The accumulation in one launch.  prev == nullptr: the first frame, which reprojects nothing whatever the carry (it is not read)
hipError_t launch_temporal_accumulate(const TemporalFrameDev& cur, const TemporalFrameDev* prev, TemporalArgs args, const TemporalCarryDev& carry,
                                      const TemporalOutsDev& outs, hipStream_t);
// The rectified accumulation of a frame WITH a previous frame in two launches: the gather into d_scratch (TEMPORAL_RECTIFY_RECORD_BYTES per
// pixel, 16-byte aligned), then the rectifying blend over those records.  radius is 1 .. 3
constexpr size_t TEMPORAL_RECTIFY_RECORD_BYTES = 32;
hipError_t launch_temporal_gather(const TemporalFrameDev& cur, const TemporalFrameDev& prev, TemporalArgs args, const TemporalCarryDev& carry, void* d_scratch,
                                  hipStream_t);
hipError_t launch_temporal_rectify_blend(const TemporalFrameDev& cur, TemporalArgs args, uint32_t radius, float gamma, const void* d_scratch, float* d_out_film,
                                         float* d_out_half, float* d_out_length, hipStream_t);
// pt_kernels_budget.hip: the sample budget by reprojected history (include/mi355pt_budget.h); the probe carries a pixel as the
// accumulation does (TemporalCarryDev).  The probe's per-tile part: the launcher fills tiles_x and n_tiles
struct BudgetTilesDev { uint32_t tiles_x, n_tiles, base_spp, max_spp; float target_history; };
// ONE launch: per pixel the history length the accumulation will gather (d_pred, nullptr: not wanted), per tile its minimum and the
// count budget_plan.hpp's formula gives.  prev == nullptr: the first frame, no G-buffer is read.  args.spp and args.half_spp are not read
hipError_t launch_budget_probe(const TemporalFrameDev& cur, const TemporalFrameDev* prev, TemporalArgs args, const TemporalCarryDev& carry, BudgetTilesDev tiles,
                               float* d_pred, float* d_tile_len, uint32_t* d_tile_spp, hipStream_t);
// TWO launches: the flags "clamped tile_spp > level_spp" into d_scratch (one u32 per tile) with H := F on the flagged tiles, then
// launch_adaptive_compact into d_list and d_count
hipError_t launch_budget_select(const float* d_film, float* d_half, uint32_t width, uint32_t height, const uint32_t* d_tile_spp, uint32_t level_spp,
                                uint32_t base_spp, uint32_t max_spp, void* d_scratch, uint32_t* d_list, uint32_t* d_count, hipStream_t);
// both films / (float)(tile_spp / 2) of the pixel's tile (in place allowed); length += tile_spp / base_spp - 1, capped, where tile_spp > base_spp
hipError_t launch_pair_normalize_tiles(const float* d_film, const float* d_half, const uint32_t* d_tile_spp, uint32_t width, uint32_t height, float* d_out_film,
                                       float* d_out_half, hipStream_t);
hipError_t launch_length_credit(float* d_length, const uint32_t* d_tile_spp, uint32_t base_spp, float max_history, uint32_t width, uint32_t height, hipStream_t);
// pt_kernels_ids.hip: the ID pass (include/mi355pt_motion.h): one primary ray through every pixel centre, instance + 1 of the closest hit or
// 0 into d_ids.  The plan must have block_log2 == 3 and chunks == 1 (api_motion.cpp, the G-buffer pass's plan): one pixel per lane
hipError_t launch_ids(const DevScene&, const DevCamera&, const DevParams&, uint32_t* d_ids, unsigned* d_counter, DevStats* d_stats, int grid, hipStream_t);
int query_resident_waves_ids();
// pt_kernels_flow.hip: the flow pass (include/mi355pt_flow.h): the ID pass's launch with a 32-byte motion record per pixel from the hit's
// triangle in d_tris_prev (the scene's mark) and in DevScene::tris_render.  d_flow is 16-byte aligned; d_ids == nullptr: not wanted;
// d_hits != nullptr (16 bytes per pixel: tri, b0, b1, b2) takes the debug twin of the kernel.  The plan is launch_ids's
hipError_t launch_flow(const DevScene&, const DevCamera&, const DevParams&, const DevTri* d_tris_prev, FlowPixelDev* d_flow, uint32_t* d_ids, void* d_hits,
                       unsigned* d_counter, DevStats* d_stats, int grid, hipStream_t);
int query_resident_waves_flow(bool debug);
// pt_kernels_upsample.hip: the guided half-resolution upsample (include/mi355pt_upsample.h): one launch on the grid of denoise_grid_blocks
// over the FULL frame.  The G-buffer sums of one resolution as the kernel takes them (albedo == nullptr: not given, then on both sides);
// low_half == nullptr: no half film (then out_half is not written).  The launcher fills UpsampleArgs::blocks_x
struct UpsampleGuidesDev { const float *albedo = nullptr, *shading_normal = nullptr, *position = nullptr, *hit = nullptr; };
struct UpsampleArgs {
    uint32_t width, height, blocks_x;      // the FULL frame, both even; the low frame is width / 2 x height / 2
    float spp, half_spp;                   // (float)spp, (float)(spp / 2)
    float spp_albedo_low, spp_albedo_full;
    float pos_tol, normal_cos, emitter_tol, min_weight, albedo_eps;
};
hipError_t launch_upsample(const float* d_low_film, const float* d_low_half, const UpsampleGuidesDev& low, const UpsampleGuidesDev& full, UpsampleArgs args,
                           float* d_out_film, float* d_out_half, hipStream_t);
// pt_kernels_display.hip: the display stage (include/mi355pt_display.h).  The meter: two launches, the block histograms of display_plan.hpp's
// plan into d_scratch (rows x 258 words, every word that is read is written first) and the one-block finish, which reads d_prev_record
// (nullptr: none; may be d_record) before it writes d_record (8 words) and, when given, d_hist (258 words).  The display: one launch, one
// thread per pixel; d_record == nullptr: E is args.exposure.  white2 and hable_white are the host's f32 white * white and h(white)
struct DisplayMeterArgs {
    uint32_t width, height;
    float spp;                              // (float)spp
    uint32_t base;                          // (log2_lum_min + 127) << 3
    uint32_t trim_low, trim_high;
    float key, e_min, e_max, adapt;
};
struct DisplayArgs {
    uint32_t width, height;
    float spp;
    uint32_t tone, encode;
    float exposure, white2, hable_white;
};
hipError_t launch_display_meter(const float* d_film, const DisplayMeterArgs& args, const uint32_t* d_prev_record, uint32_t* d_scratch, uint32_t* d_record,
                                uint32_t* d_hist, hipStream_t);
// ... and its two launches one by one (mi355pt_probe_display_meter_ms times them apart)
hipError_t launch_display_hist(const float* d_film, const DisplayMeterArgs& args, uint32_t* d_scratch, hipStream_t);
hipError_t launch_display_finish(const uint32_t* d_scratch, const DisplayMeterArgs& args, const uint32_t* d_prev_record, uint32_t* d_record, uint32_t* d_hist, hipStream_t);
hipError_t launch_display(const float* d_film, const DisplayArgs& args, const uint32_t* d_record, float* d_out, hipStream_t);
float display_hable(float x);      // h(x) of the header on the host, the same single-rounded steps as the kernel
// pt_kernels_bloom.hip: the bloom stage (include/mi355pt_bloom.h) over bloom_plan.hpp's plan: 2 x levels launches on one stream — the
// reductions 0 -> 1 (with the bright pass and, with firefly, the weights) .. L - 1 -> L into d_scratch (16-byte records, 16-byte aligned;
// every word that is read is written first), the expansions L -> L - 1 .. 2 -> 1 in place over the levels, and the composite into d_out,
// which may be d_film.  d_record == nullptr: E is args.exposure.  s0 is the host's f32 1 - scatter
struct BloomArgs {
    uint32_t width, height, levels, firefly;
    float spp;                              // (float)spp
    float threshold, knee, exposure;
    float s0, s1, base, intensity;
};
hipError_t launch_bloom(const float* d_film, const BloomArgs& args, const uint32_t* d_record, void* d_scratch, float* d_out, hipStream_t);
// pt_kernels_robust.hip: the robust film (include/mi355pt_robust.h): one launch, one thread per pixel, over n_buckets in {4, 8, 16, 32} films
// of args.pixels x 3 floats at d_buckets.  d_out_half == nullptr: single output (one set of n_buckets); otherwise pair output (two sets of
// n_buckets / 2).  d_out_trim == nullptr: not wanted.  The frame has fewer than 2^32 pixels
struct RobustArgs {
    uint64_t pixels;
    float spp;                              // (float)spp_bucket
    float inv_spp;                          // 1 / spp where spp_bucket is a power of two (exact), 0 otherwise: the kernel divides
    uint32_t mode;                          // MI355PT_ROBUST_*
    float gini_scale;
};
hipError_t launch_robust_combine(const float* d_buckets, uint32_t n_buckets, const RobustArgs& args, float* d_out, float* d_out_half, uint8_t* d_out_trim, hipStream_t);
// pt_kernels_rebase.hip: a camera move on a built scene (include/mi355pt_rebase.h, scene_rebase.cpp; every launch below from scene_update.cpp).  launch_rebase_tris: the render-space
// positions of all n_tris leaf-order triangles from the local records and the instance matrices; count_degenerate adds the number of
// triangles whose cross product is exactly zero to *d_degenerate_count (which the caller has cleared).  launch_refit_bvh2_height: the boxes of
// the `count` (node, side) entries from d_entries[first] on — ONE height group of rebase_plan.hpp's plan; the caller launches the groups
// lowest first on one stream.  launch_refit_nodes4: every used slot of the 4-wide tree from its source in the refit BVH2, padded
hipError_t launch_rebase_tris(const DevTriLocal* d_local, const DevInstance* d_instances, DevTri* d_render, uint32_t n_tris, bool count_degenerate,
                              uint32_t* d_degenerate_count, hipStream_t);
hipError_t launch_refit_bvh2_height(DevNode* d_nodes, const DevTri* d_tris_render, const uint32_t* d_entries, uint32_t first, uint32_t count, hipStream_t);
hipError_t launch_refit_nodes4(DevNode4* d_nodes4, const DevNode* d_nodes, const uint32_t* d_slot_src, uint32_t n_slots, int32_t root, hipStream_t);
// pt_kernels_instances.hip: an instance move on a built scene (include/mi355pt_instances.h, scene_instances.cpp; launched from scene_update.cpp).  launch_shade_refresh: ng
// and light_pdf_area of the leaf-order shading records whose instance has its bit set in d_moved_bits ((n_instances + 31) / 32 words);
// d_light_pdf: light_pdf_area per light triangle, indexed DevLight::first_tri + local_tri.  launch_sah_cost: TWO launches, the block sums of
// the terms of all n_entries plan entries and the one-block finish; d_scratch holds sah_scratch_floats(n_entries) floats and receives
// {cost, sum of the terms, half area of the root} in its first three
hipError_t launch_shade_refresh(DevTriShade* d_shade, const DevTriLocal* d_local, const DevInstance* d_instances, const uint32_t* d_moved_bits, const DevLight* d_lights,
                                const float* d_light_pdf, uint32_t n_tris, uint32_t n_instances, uint32_t n_lights, uint32_t n_light_pdf, hipStream_t);
size_t sah_scratch_floats(uint32_t n_entries);
hipError_t launch_sah_cost(const DevNode* d_nodes, int32_t root, const uint32_t* d_entries, uint32_t n_entries, float* d_scratch, hipStream_t);
constexpr uint32_t SAH_COST_LAUNCHES = 2;
// pt_kernels_deform.hip: a mesh deformation on a built scene (include/mi355pt_deform.h, scene_deform.cpp; launched from scene_update.cpp).  launch_deform_tris: the positions
// of the local records and rows 0 - 2 of the shading records of the leaf-order triangles whose instance has a slot in d_table
// (deform_plan.hpp deform_table: n_instances words, then from word slots_at on n_slots slot records), gathered from d_staging through the
// index pool d_mesh_idx; the triangles of every other instance are not written
hipError_t launch_deform_tris(DevTriLocal* d_local, DevTriShade* d_shade, const uint32_t* d_table, const float* d_staging, const uint32_t* d_mesh_idx, uint32_t n_tris,
                              uint32_t n_instances, uint32_t slots_at, uint32_t n_slots, hipStream_t);
// pt_kernels_edit.hip: a material edit on a built scene (include/mi355pt_edit.h, scene_edit.cpp; launched from scene_update.cpp).  launch_reclass_tris: the class word of
// the leaf-order triangles whose material has a class in d_table (scene_edit_plan.hpp edit_class_table: n_materials words, EDIT_CLASS_UNCHANGED
// = not written), in d_local, in d_render and, where it is given, in d_walked (DevScene::tris when it is neither of the two; nullptr otherwise)
hipError_t launch_reclass_tris(DevTriLocal* d_local, DevTri* d_render, DevTri* d_walked, const DevTriShade* d_shade, const uint32_t* d_table, uint32_t n_tris,
                               uint32_t n_materials, hipStream_t);

// Resident 64-thread blocks (= waves) of `kernel` on the current device: the persistent grid size of the EXACT instantiation a launch takes
// (the register count, and so the occupancy, differs between instantiations and between translation units with their own backend flags).
// per_cu <= 0 (no answer): 8 blocks per CU.
inline int resident_waves_per_device(int per_cu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 2048;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 2048;
    return prop.multiProcessorCount * (per_cu > 0 ? per_cu : 8);
}
template <typename Kernel>
int resident_waves_of(Kernel kernel) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess) per_cu = 0;
    return resident_waves_per_device(per_cu);
}

}  // namespace pt
