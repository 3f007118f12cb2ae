// What the host translation units behind the C ABI share (api.cpp and the api_<stage>.cpp files, one per public header; scene_rebase.cpp,
// scene_instances.cpp, scene_deform.cpp, scene_update.cpp, scene_debug.cpp): the scene object and its launch context, fail / HIP_TRY, the device buffer and event holders, what api.cpp
// defines for the others, and api_temporal.cpp's driver of the temporal accumulations.  The pure argument predicates are api_checks.hpp.  Not installed, not an ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mi355pt.h"
#include "api_checks.hpp"
#include "launch.hpp"
#include "launch_plan.hpp"
#include "scene.hpp"

namespace pt {

// Per-scene launch resources, allocated once (no hipMalloc/hipFree/sync on the launch path, so a caller can queue
// launches on its own stream or capture them): the MurmurHash(dimension, seed) table per seed and a ring of work
// counters / stats blocks so that back-to-back asynchronous launches never share a counter.
constexpr int CTX_RING = 16;
struct LaunchCtx {
    int device = -1;                  // the device every buffer below lives on (= SceneImpl::device when the context was made)
    int waves[2][2][3] = {{{0}}};     // [instrumented][sampler][strategy]: resident waves of the kernel that combination launches (0: not asked yet)
    int aov_waves[3] = {0, 0, 0};     // [MI355PT_AOV_*]: the same for the AOV kernel of this scene's feature set
    int gbuffer_waves = 0;            // ... and for the G-buffer kernel (pt_kernels_gbuffer.hip)
    int ids_waves = 0;                // ... and for the ID pass (pt_kernels_ids.hip)
    int flow_waves[2] = {0, 0};       // ... and for the flow pass (pt_kernels_flow.hip): [0] the production kernel, [1] its debug twin
    uint64_t* d_hash = nullptr;
    uint32_t hash_seed = 0;
    bool hash_valid = false;
    unsigned* d_counters = nullptr;   // CTX_RING counters
    DevStats* d_stats = nullptr;      // CTX_RING blocks
    float* d_defer = nullptr;         // the resident waves' queues (pt_kernel.hpp queue_bytes_per_wave: 24 / 40 / 16 KB per wave by kernel), sized for the largest launch seen
    size_t defer_bytes = 0;
    float* d_partial = nullptr;       // per-chunk film tiles of split launches (tiles * chunks * 64 * 3 floats), grown on demand;
    size_t partial_bytes = 0;         // reused by consecutive launches: one stream at a time per scene
    uint32_t* d_tiles = nullptr;      // mi355pt_render_accum_tiles_device: the caller's host list on the device, grown on demand
    size_t tiles_bytes = 0;
    int next = 0;
    ~LaunchCtx() {
        // freed with the owning device current (a scene rebuilt on another device drops its context from there)
        int cur = -1;
        const bool swap = device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
        (void)hipFree(d_hash); (void)hipFree(d_counters); (void)hipFree(d_stats); (void)hipFree(d_partial); (void)hipFree(d_defer); (void)hipFree(d_tiles);
        if (swap) (void)hipSetDevice(cur);
    }
};
// One device's share of a multi-device scene (mi355pt_scene_build_multi): a full replica of the scene on that device plus
// the stream, film and event mi355pt_render_multi drives it with.  Replica 0 is the scene object itself.
struct MultiPart {
    int device = -1;
    mi355pt_scene* scene = nullptr;      // owned unless it is the parent (part 0)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    float* d_film = nullptr;             // full-frame linear film of this device's tile shard
    float* d_pack = nullptr;             // parts 1..: the shard's tiles as a compact film (tile-major, 192 floats per tile) — what crosses xGMI
    float* d_stage = nullptr;            // part 0 only: one landing area per peer for those compact films
    float* d_out = nullptr;              // part 0 only: resolved frame
    size_t film_floats = 0, pack_floats = 0, stage_floats = 0;
};

}  // namespace pt

struct mi355pt_scene {
    pt::SceneImpl impl;
    mutable pt::LaunchCtx* ctx = nullptr;
    mutable std::vector<pt::MultiPart> parts;   // empty unless built with mi355pt_scene_build_multi
    ~mi355pt_scene();
};

namespace pt {

extern bool g_debug_unlocked;      // mi355pt_debug_unlock: lets mi355pt_params.rr_gate_slack through
void cie_cmf4(float out[470 * 4]);   // the CIE colour matching functions SceneImpl::build takes: [470][4] (xbar, ybar, zbar, 0) (api.cpp)
int fail(int code, const std::string& msg);   // sets the thread's mi355pt_last_error (api.cpp) and returns `code`
// api_scene.cpp: the validators mi355pt_scene_add_material / mi355pt_scene_add_delta_light share with mi355pt_scene_edit (scene_edit.cpp):
// the descriptor as the description's record (the light's: its hidden emissive material), or the refusal's code with its text in *err
int lower_material_desc(const SceneImpl& im, const mi355pt_material_desc& d, DevMaterial* out, std::string* err);
int lower_light_desc(const SceneImpl& im, const mi355pt_light_desc& d, DevMaterial* hidden, std::string* err);
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return fail(MI355PT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// A device buffer of a host-buffer entry point, freed with the object, and that entry point's staging: synchronous copies on the null
// stream.  An input the caller did not give and an output it does not want stay null pointers, which is what the _device twin takes for them
template <typename T>
struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    // each does nothing when `host` is null: the device copy of host[0 .. n); n elements for an output wanted in `host`; p[0 .. n) into `host`
    hipError_t upload(const T* host, size_t n) {
        const hipError_t e = alloc_for(host, n);
        return !host || e != hipSuccess ? e : hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t alloc_for(const T* host, size_t n) { return host ? alloc(n) : hipSuccess; }
    hipError_t download(T* host, size_t n) const { return host ? hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
};

// A buffer of the updates in place (scene_update.cpp), allocated by the first update after a build that needs it and freed with the scene
template <typename T>
hipError_t ensure(SceneImpl* s, T** p, size_t count) {
    if (*p) return hipSuccess;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 16));
    if (e != hipSuccess) return e;
    s->allocs.push_back(q);
    *p = (T*)q;
    return hipSuccess;
}

// A HIP event, destroyed with the object: an error between create() and the end of the scope does not leak it
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return hipEventCreate(&e); }
    hipError_t record(hipStream_t stream) { return hipEventRecord(e, stream); }
    hipError_t synchronize() { return hipEventSynchronize(e); }
    hipError_t elapsed_ms(const Event& since, float* ms) const { return hipEventElapsedTime(ms, since.e, e); }
};

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }   // host_ms of an entry point
// `aov`: the AOV renderers ignore strategy and max_depth (mi355pt_render_aov), so they are not checked for them
int check_args(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, bool aov = false);
// aov_kind < 0: the path-tracing kernels; MI355PT_AOV_*: the AOV kernel (pt_kernels_aov.hip) over the same work items and work counter —
// but never a split sample range —, with `illuminant_lut` for the albedo kind
int render_accum_range(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end,
                       float* d_accum, void* hip_stream, mi355pt_stats* stats, const PathOut& pout, int aov_kind = -1, uint32_t illuminant_lut = 0);
// what the tile-list entry and the adaptive driver ask of (scene, camera, params) beyond check_args
int check_tiles_args(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p);
// the scene's launch context with the hash table valid for `seed`; `slot` receives a fresh ring slot
int get_launch_ctx(const mi355pt_scene* sc, uint32_t seed, LaunchCtx** out, int* slot);
// the launches of [s_begin, s_end) into d_accum, arguments checked; with d_list, of the tiles d_list[0 .. n_list) (device memory)
int launch_ranges(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, float* d_accum,
                  hipStream_t stream, mi355pt_stats* stats, const uint32_t* d_list, uint32_t n_list,
                  const PathOut& pout = PathOut{nullptr, nullptr, nullptr, 0u, 0u}, int aov_kind = -1, uint32_t illuminant_lut = 0);
// What every launch over a ring slot of `lc` shares: the slot's work counter zeroed on `stream`, then launch(d_counter, d_stats), which
// returns an MI355PT_* code.  stats == NULL: nothing else, fully asynchronous.  Otherwise events around the launch, a wait for it, and
// *stats = {kernel_ms, launches = 1}; with `counts` the slot's DevStats block is zeroed before the launch and read into *stats after it
int timed_launch(LaunchCtx* lc, int slot, hipStream_t stream, mi355pt_stats* stats, bool counts,
                 const std::function<int(unsigned* d_counter, DevStats* d_stats)>& launch);
// api_temporal.cpp: the one driver behind the twelve mi355pt_temporal_accumulate* entry points of mi355pt_temporal.h,
// mi355pt_temporal_rectify.h, mi355pt_motion.h and mi355pt_flow.h.  A call is its base arguments ...
struct TemporalCall {
    const mi355pt_temporal_frame* cur; uint32_t spp; const mi355pt_temporal_frame* prev; const mi355pt_temporal_view* view; uint32_t width, height;
    const mi355pt_temporal_params* tp; float *out_film, *out_half, *out_length;
};
// ... how a pixel's hit is carried one frame back: by the view alone, through the per-instance table or through the per-pixel records
// (`align`: what is asked of the table or the records, 16 for a device form, 1 for a host form) ...
struct TemporalCarry {
    enum Kind { NONE = CARRY_STATIC, TABLE = CARRY_TABLE, FLOW = CARRY_FLOW } kind = NONE;
    const uint32_t *ids_cur = nullptr, *ids_prev = nullptr;
    const mi355pt_motion_xform* table = nullptr; uint32_t n_entries = 0;
    const mi355pt_flow_pixel* flow = nullptr;
    size_t align = 1;
};
// a checked carry whose buffers are on the device, as the kernels and the budget's probe take it
inline TemporalCarryDev carry_dev(const TemporalCarry& c) {
    TemporalCarryDev d;
    d.kind = (TemporalCarryKind)c.kind;
    d.ids_cur = c.ids_cur; d.ids_prev = c.ids_prev;
    d.table = (const MotionXformDev*)c.table; d.last_entry = c.table ? c.n_entries - 1u : 0u;
    d.flow = (const FlowPixelDev*)c.flow;
    return d;
}
// ... and, for a rectified form, its parameters (a host form has no scratch: the driver allocates one)
struct TemporalRectify { const mi355pt_temporal_rectify_params* rp; void* scratch = nullptr; size_t scratch_bytes = 0; };
// The checks in their one order — temporal_check, the rectify parameters, the scratch (device form), the carry's own —, then the launches on
// `hip_stream`, or the host form's staging around them on the null stream.  rect == nullptr: not rectified
int temporal_accumulate_device(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect, void* hip_stream);
int temporal_accumulate_host(const TemporalCall& c, const TemporalCarry& carry, const TemporalRectify* rect);
// the carries' own checks (api_motion.cpp, api_flow.cpp); scratch: the rectified device form's, which counts among the outputs, or nullptr
int motion_check(const TemporalCarry& carry, const TemporalCall& c, const void* scratch);
int flow_in_check(const TemporalCarry& carry, const TemporalCall& c, const void* scratch);
// api_motion.cpp, for api_flow.cpp and api_debug.cpp, whose flow pass is the ID pass's launch: every check of mi355pt_render_ids[_device]
// (`out`: the per-pixel output buffer) and the launch's shape
int ids_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const void* out);
LaunchPlan plan_ids(const mi355pt_camera* cam, const mi355pt_params* p, int waves);
// api_flow.cpp, for api_debug.cpp's mi355pt_render_flow_debug: the checks and the launch of mi355pt_render_flow_device; with d_hits the
// kernel's debug twin, which also writes 16 bytes per pixel there
int flow_check(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const void* flow, size_t flow_align, const void* ids);
int render_flow_launch(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, mi355pt_flow_pixel* d_flow, uint32_t* d_ids, void* d_hits,
                       void* hip_stream, mi355pt_stats* stats);

}  // namespace pt
