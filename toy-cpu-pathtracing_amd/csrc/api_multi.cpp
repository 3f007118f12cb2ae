// Several GPUs of one node behind ONE call (include/mi355pt.h: mi355pt_scene_build_multi, mi355pt_render_multi) and the scene's destructor.
// The reference calls the seam once from one process (renderer/src/main.rs:228).  mi355pt_scene_build_multi replicates the scene
// on every listed device (the working set is < 30 MB); mi355pt_render_multi deals the frame's 8x8 tiles round-robin to the devices
// (each launch on its own stream, concurrently), gathers the rank-local linear films onto the first device over xGMI peer copies
// and adds them there — the tile shards are disjoint, so the sum is exact and its order fixed — then resolves and copies out.
// No communicator is needed inside one process; the one-process-per-GPU path (bench.py, torch.distributed) reduces the same films
// with RCCL.
#include <new>

#include "api_internal.hpp"

using namespace pt;

static void free_parts(std::vector<MultiPart>& parts) {
    for (size_t i = 0; i < parts.size(); ++i) {
        MultiPart& m = parts[i];
        (void)hipSetDevice(m.device);
        if (m.stream) (void)hipStreamDestroy(m.stream);
        if (m.done) (void)hipEventDestroy(m.done);
        (void)hipFree(m.d_film); (void)hipFree(m.d_pack); (void)hipFree(m.d_stage); (void)hipFree(m.d_out);
        if (i > 0) delete m.scene;
    }
    parts.clear();
}
mi355pt_scene::~mi355pt_scene() {
    int cur = 0;
    const bool have = !parts.empty() && hipGetDevice(&cur) == hipSuccess;
    free_parts(parts);
    if (have) (void)hipSetDevice(cur);
    delete ctx;
}

extern "C" {

int mi355pt_scene_build_multi(mi355pt_scene* s, const mi355pt_camera* cam, int n_devices, const int* device_ids) {
    if (!s || !cam || !device_ids || n_devices < 1 || n_devices > 64) return fail(MI355PT_E_INVALID, "bad device list");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MI355PT_E_NO_DEVICE, "no HIP device: the product path requires a gfx950 GPU");
    for (int i = 0; i < n_devices; ++i) if (device_ids[i] < 0 || device_ids[i] >= ndev) return fail(MI355PT_E_INVALID, "device id out of range");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    free_parts(s->parts);
    int rc = MI355PT_OK;
    std::vector<MultiPart> parts((size_t)n_devices);
    for (int i = 0; i < n_devices && rc == MI355PT_OK; ++i) {
        MultiPart& m = parts[(size_t)i];
        m.device = device_ids[i];
        if (hipSetDevice(m.device) != hipSuccess) { rc = fail(MI355PT_E_DEVICE, "hipSetDevice failed"); break; }
        if (i == 0) m.scene = s;
        else {
            m.scene = new (std::nothrow) mi355pt_scene();
            if (!m.scene) { rc = fail(MI355PT_E_INVALID, "allocation failed"); break; }
            SceneImpl& d = m.scene->impl; const SceneImpl& o = s->impl;       // the description, not the lowered state
            d.table = o.table; d.luts = o.luts; d.textures = o.textures; d.meshes = o.meshes; d.materials = o.materials;
            d.instances = o.instances; d.envs = o.envs; d.delta_lights = o.delta_lights; d.bvh_builder = o.bvh_builder; d.lowering = o.lowering;
        }
        rc = mi355pt_scene_build(m.scene, cam);
        if (rc == MI355PT_OK && hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking) != hipSuccess) rc = fail(MI355PT_E_DEVICE, "hipStreamCreate failed");
        if (rc == MI355PT_OK && hipEventCreateWithFlags(&m.done, hipEventDisableTiming) != hipSuccess) rc = fail(MI355PT_E_DEVICE, "hipEventCreate failed");
        if (rc == MI355PT_OK && i > 0 && m.device != parts[0].device) {
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, parts[0].device, m.device);
            if (can) { (void)hipSetDevice(parts[0].device); (void)hipDeviceEnablePeerAccess(m.device, 0); (void)hipGetLastError(); }   // already enabled is fine
        }
    }
    (void)hipSetDevice(cur);
    if (rc != MI355PT_OK) { const std::string keep = mi355pt_last_error(); free_parts(parts); return fail(rc, keep); }   // (the error of the step that failed)
    s->parts = std::move(parts);
    return MI355PT_OK;
}

int mi355pt_render_multi(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, float* out_rgb) {
    if (!s || !cam || !p || !out_rgb) return fail(MI355PT_E_INVALID, "null argument");
    if (s->parts.empty()) return fail(MI355PT_E_NOT_BUILT, "scene not built with mi355pt_scene_build_multi");
    if (p->shard_count > 1) return fail(MI355PT_E_INVALID, "mi355pt_render_multi shards the frame itself: pass shard_count 0 or 1");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "collect_stats is a single-device diagnostic");
    if (cam->width == 0 || cam->height == 0 || p->spp == 0) return fail(MI355PT_E_INVALID, "empty image or spp == 0");
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    std::vector<MultiPart>& parts = s->parts;
    const uint32_t n = (uint32_t)parts.size();
    const size_t film = (size_t)cam->width * cam->height * 3, film_pad = (film + 3) / 4 * 4;
    int rc = MI355PT_OK;
    auto hip_ok = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == MI355PT_OK) rc = fail(MI355PT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); return e == hipSuccess; };
    // the shards: device i renders frame tiles i, i + n, i + 2 n, ...; its share of the film is tiles_of(i) * 192 floats
    auto tiles_of = [&](uint32_t i) { return shard_tile_count(cam->width, cam->height, i, n); };
    std::vector<size_t> stage_off(n, 0);
    size_t stage_total = 0;
    for (uint32_t i = 1; i < n; ++i) { stage_off[i] = stage_total; stage_total += (size_t)tiles_of(i) * 192u; }
    // 1. every device renders its tile shard into its own zeroed film, concurrently; a peer then packs its tiles and PUSHES the compact
    //    film (film / n bytes) into its own landing area on the first device, on its own stream: the n - 1 transfers overlap each other
    //    and the first device's rendering
    {
        MultiPart& r = parts[0];
        if (hip_ok(hipSetDevice(r.device), "hipSetDevice") && r.stage_floats < stage_total) {
            (void)hipFree(r.d_stage); r.d_stage = nullptr; r.stage_floats = 0;
            if (hip_ok(hipMalloc((void**)&r.d_stage, stage_total * sizeof(float)), "hipMalloc stage")) r.stage_floats = stage_total;
        }
    }
    for (uint32_t i = 0; i < n && rc == MI355PT_OK; ++i) {
        MultiPart& m = parts[i];
        if (!hip_ok(hipSetDevice(m.device), "hipSetDevice")) break;
        if (m.film_floats != film_pad) {
            (void)hipFree(m.d_film); (void)hipFree(m.d_out); m.d_film = m.d_out = nullptr; m.film_floats = 0;
            if (!hip_ok(hipMalloc((void**)&m.d_film, film_pad * sizeof(float)), "hipMalloc film")) break;
            if (i == 0 && !hip_ok(hipMalloc((void**)&m.d_out, film_pad * sizeof(float)), "hipMalloc out")) break;
            m.film_floats = film_pad;
        }
        const size_t pack = (size_t)tiles_of(i) * 192u;
        if (i > 0 && m.pack_floats < pack) {
            (void)hipFree(m.d_pack); m.d_pack = nullptr; m.pack_floats = 0;
            if (!hip_ok(hipMalloc((void**)&m.d_pack, std::max<size_t>(pack, 1) * sizeof(float)), "hipMalloc pack")) break;
            m.pack_floats = pack;
        }
        if (!hip_ok(hipMemsetAsync(m.d_film, 0, film_pad * sizeof(float), m.stream), "hipMemsetAsync")) break;
        mi355pt_params q = *p;
        q.shard_index = i; q.shard_count = n;
        if ((rc = mi355pt_render_accum_device(m.scene, cam, &q, 0, p->spp, m.d_film, (void*)m.stream, nullptr))) break;
        if (i > 0 && pack) {
            if (!hip_ok(launch_film_pack(m.d_film, cam->width, cam->height, i, n, tiles_of(i), m.d_pack, m.stream), "film pack")) break;
            if (!hip_ok(hipMemcpyPeerAsync(parts[0].d_stage + stage_off[i], parts[0].device, m.d_pack, m.device, pack * sizeof(float), m.stream), "hipMemcpyPeerAsync")) break;
        }
        hip_ok(hipEventRecord(m.done, m.stream), "hipEventRecord");
    }
    // 2. on the first device: each landed shard is written into the film (disjoint tiles: stores in a fixed order, exact and
    //    deterministic), then resolve and copy out
    if (rc == MI355PT_OK && hip_ok(hipSetDevice(parts[0].device), "hipSetDevice")) {
        MultiPart& r = parts[0];
        for (uint32_t i = 1; i < n && rc == MI355PT_OK; ++i) {
            if (!tiles_of(i)) continue;
            if (!hip_ok(hipStreamWaitEvent(r.stream, parts[i].done, 0), "hipStreamWaitEvent")) break;
            hip_ok(launch_film_unpack(r.d_film, cam->width, cam->height, i, n, tiles_of(i), r.d_stage + stage_off[i], r.stream), "film unpack");
        }
        if (rc == MI355PT_OK) rc = mi355pt_film_resolve_device(r.d_film, cam->width * cam->height, p->spp, r.d_out, (void*)r.stream);
        if (rc == MI355PT_OK) hip_ok(hipMemcpyAsync(out_rgb, r.d_out, film * sizeof(float), hipMemcpyDeviceToHost, r.stream), "hipMemcpyAsync");
        if (rc == MI355PT_OK) hip_ok(hipStreamSynchronize(r.stream), "hipStreamSynchronize");
    }
    if (rc != MI355PT_OK) for (MultiPart& m : parts) { (void)hipSetDevice(m.device); (void)hipStreamSynchronize(m.stream); }   // nothing of this call stays in flight
    (void)hipSetDevice(cur);
    return rc;
}

}  // extern "C"
