// The mi355pt_debug.h surface of libmi355pt.so: probes, the per-sample log, diagnostic switches.  Host C++ only, like api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "api_internal.hpp"
#include "camera_candidates.hpp"
#include "scene_lower.hpp"

using namespace pt;

extern "C" {

int mi355pt_debug_unlock(int on) { const int was = g_debug_unlocked ? 1 : 0; g_debug_unlocked = on != 0; return was; }

int mi355pt_scene_debug_set_lowering(mi355pt_scene* s, int mode) {
    if (!s) return fail(MI355PT_E_INVALID, "null argument");
    if (mode < 0 || mode > 2) return fail(MI355PT_E_INVALID, "unknown lowering mode");
    s->impl.lowering = mode;
    return MI355PT_OK;
}

int mi355pt_scene_debug_lowering_digest(const mi355pt_scene* s, const mi355pt_camera* cam, char* names_buf, size_t names_len, uint64_t* digests, uint32_t* n) {
    if (!s || !cam || !names_buf || !digests || !n) return fail(MI355PT_E_INVALID, "null argument");
    // SceneImpl::build without its three device steps: no query, the host builder, no upload
    std::string err;
    int rc;
    LoweredGeometry geo; BvhOut bvh; LoweredScene ls; LowerReport rep;
    if ((rc = lower_geometry(s->impl, cam, &geo, &err))) return fail(rc, err);
    build_bvh(geo.build_tris, &bvh);
    if (bvh.max_depth >= STACK_DEPTH) return fail(MI355PT_E_INVALID, "BVH deeper than the traversal stack");
    float cmf[470 * 4];
    cie_cmf4(cmf);
    if ((rc = lower_scene(s->impl, std::move(geo), std::move(bvh), cmf, &ls, &rep, &err)) || (rc = lower_tree4(&ls, &rep, &err))) return fail(rc, err);
    std::vector<std::string> names; std::vector<uint64_t> dig;
    lowering_digests(ls, rep, &names, &dig);
    std::string text;
    for (const std::string& nm : names) text += nm + "\n";
    text += lowering_info(ls, rep, false, nullptr);
    const uint32_t cap = *n;
    *n = (uint32_t)dig.size();
    if (cap < dig.size() || names_len < text.size() + 1) return fail(MI355PT_E_INVALID, "digest or name buffer too small");
    std::memcpy(digests, dig.data(), dig.size() * sizeof(uint64_t));
    std::memcpy(names_buf, text.c_str(), text.size() + 1);
    return MI355PT_OK;
}

int mi355pt_scene_debug_camera_candidates(const mi355pt_scene* s, const mi355pt_camera* cam, const uint32_t* rects, uint32_t n_rects, uint32_t cap,
                                          uint32_t* out_counts, uint8_t* out_overflow, uint32_t* out_indices, float* out_tris, uint32_t* n_tris) {
    if (!s || !cam || (n_rects && (!rects || !out_counts || !out_overflow))) return fail(MI355PT_E_INVALID, "null argument");
    if (cap < 1u || cap > 4096u) return fail(MI355PT_E_INVALID, "cap must be 1 .. 4096");
    if (PT_NODE_Q16) return fail(MI355PT_E_INVALID, "the candidate walk reads the float 4-wide tree");
    // the lowering of mi355pt_scene_debug_lowering_digest: host builder, nothing uploaded
    std::string err;
    int rc;
    LoweredGeometry geo; BvhOut bvh; LoweredScene ls; LowerReport rep;
    if ((rc = lower_geometry(s->impl, cam, &geo, &err))) return fail(rc, err);
    build_bvh(geo.build_tris, &bvh);
    if (bvh.max_depth >= STACK_DEPTH) return fail(MI355PT_E_INVALID, "BVH deeper than the traversal stack");
    float cmf[470 * 4];
    cie_cmf4(cmf);
    if ((rc = lower_scene(s->impl, std::move(geo), std::move(bvh), cmf, &ls, &rep, &err)) || (rc = lower_tree4(&ls, &rep, &err))) return fail(rc, err);
    const uint32_t n = (uint32_t)ls.tris_render.size();
    if (out_tris) {
        if (!n_tris || *n_tris < n) return fail(MI355PT_E_INVALID, "triangle buffer too small");
        for (uint32_t i = 0; i < n; ++i) std::memcpy(out_tris + 9 * (size_t)i, &ls.tris_render[i], 9 * sizeof(float));    // p0, p1, p2: the record's first 36 bytes
    }
    if (n_tris) *n_tris = n;
#if !PT_NODE_Q16
    const DevCamera dc = make_camera(cam);
    const DevTri* tris = ls.dev.tris_are_local ? ls.tris_local.data() : ls.tris_render.data();      // DevScene::tris (scene.cpp upload)
    uint32_t stack[CAM_WALK_STACK];
    std::vector<uint32_t> list(cap);
    for (uint32_t r = 0; r < n_rects; ++r) {
        const uint32_t* q = rects + 4 * (size_t)r;
        const CamWalk w = cam_walk(ls.nodes4.data(), ls.dev.root4, tris, ls.dev.tri_shift, cam_pyramid(dc, q[0], q[1], q[2], q[3]), list.data(), cap, stack);
        out_counts[r] = w.count; out_overflow[r] = w.overflow ? 1 : 0;
        if (out_indices) std::memcpy(out_indices + (size_t)r * cap, list.data(), sizeof(uint32_t) * w.count);
    }
#endif
    return MI355PT_OK;
}

int mi355pt_sample_log_records(const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end, size_t* out_records) {
    if (!cam || !p || !out_records || s_end <= s_begin) return fail(MI355PT_E_INVALID, "bad argument");
    *out_records = (size_t)shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) * 64u * (s_end - s_begin);
    return MI355PT_OK;
}

int mi355pt_render_sample_log(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, uint32_t s_begin, uint32_t s_end,
                              float* out_L, float* out_lambda, float* out_pdf, size_t n_records, float* out_accum) {
    int rc = check_args(s, cam, p);
    if (rc) return rc;
    if (!out_L || !out_lambda || !out_pdf || s_end > p->spp || s_begin >= s_end) return fail(MI355PT_E_INVALID, "bad sample range or null output");
    if (p->spp & (p->spp - 1u)) return fail(MI355PT_E_INVALID, "the per-sample log needs a power-of-two spp (the sample index is read back from the Morton index)");
    if (p->collect_stats) return fail(MI355PT_E_INVALID, "the per-sample log is written by the production kernel, not the instrumented one");
    const size_t need = (size_t)shard_tile_count(cam->width, cam->height, p->shard_index, p->shard_count) * 64u * (s_end - s_begin);
    if (n_records != need) return fail(MI355PT_E_INVALID, "n_records must be tiles of the shard * 64 * (sample_end - sample_begin)");
    if (need == 0) return MI355PT_OK;
    const size_t n_film = (size_t)cam->width * cam->height * 3;
    DevBuf<float> d_L, d_lam, d_pdf, d_acc;
    HIP_TRY(d_L.alloc(need * 4)); HIP_TRY(d_lam.alloc(need * 4)); HIP_TRY(d_pdf.alloc(need * 4)); HIP_TRY(d_acc.alloc(n_film));
    HIP_TRY(hipMemset(d_L.p, 0, need * 16)); HIP_TRY(hipMemset(d_lam.p, 0, need * 16)); HIP_TRY(hipMemset(d_pdf.p, 0, need * 16));
    HIP_TRY(hipMemset(d_acc.p, 0, n_film * sizeof(float)));
    if ((rc = render_accum_range(s, cam, p, s_begin, s_end, d_acc.p, nullptr, nullptr, PathOut{d_L.p, d_lam.p, d_pdf.p, s_begin, s_end - s_begin}))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_L, d_L.p, need * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_lambda, d_lam.p, need * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_pdf, d_pdf.p, need * 16, hipMemcpyDeviceToHost));
    if (out_accum) HIP_TRY(hipMemcpy(out_accum, d_acc.p, n_film * sizeof(float), hipMemcpyDeviceToHost));
    return MI355PT_OK;
}

// ---------------- probes ----------------

int mi355pt_probe_sobol(uint32_t width, uint32_t height, uint32_t spp, uint32_t seed, const uint32_t* xys, uint32_t n, const char* pattern,
                        uint32_t* out_bits) {
    if (!xys || !pattern || !out_bits || spp == 0) return fail(MI355PT_E_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MI355PT_E_NO_DEVICE, "no HIP device");
    uint32_t n_pat = (uint32_t)std::strlen(pattern), per = 0;
    for (uint32_t i = 0; i < n_pat; ++i) per += pattern[i] == '2' ? 2 : 1;
    if (n == 0 || per == 0) return MI355PT_OK;
    uint32_t log2_spp = log2_int(spp);
    uint32_t nb4 = log2_int(round_up_pow2(std::max(width, height))) + (log2_spp + 1) / 2;
    DevBuf<uint32_t> d_xys, d_out; DevBuf<uint8_t> d_pat;
    HIP_TRY(d_xys.upload(xys, (size_t)n * 3)); HIP_TRY(d_pat.upload((const uint8_t*)pattern, n_pat)); HIP_TRY(d_out.alloc((size_t)n * per));
    HIP_TRY(launch_probe_sobol(width, seed, log2_spp, nb4, d_xys.p, n, d_pat.p, n_pat, per, d_out.p, nullptr));
    HIP_TRY(d_out.download(out_bits, (size_t)n * per));
    return MI355PT_OK;
}

// Host-only: sweep-SAH BVH2 over n triangles + the BVH4 collapse, both walked on the CPU for n_rays rays (closest hit over the triangle
// boxes' entry distances is not the point — the point is that both trees return the SAME set of leaves for every ray, i.e. the collapse
// loses nothing, and that the collapsed tree's worst-case stack need stays inside STACK_DEPTH).  No device involved.
int mi355pt_probe_bvh_collapse_nodes(const void* bvh2_nodes, uint32_t n_nodes, int32_t root, uint32_t n_tris, uint32_t* out_info) {
    if (!bvh2_nodes || !out_info || n_nodes == 0) return fail(MI355PT_E_INVALID, "bad argument");
    // the same checks SceneImpl::build makes before it uploads a tree: links in range (collapse_bvh4 indexes with them), then the collapse
    // with its validation of the result (every triangle in one leaf, no cycle, worst-case per-lane stack need < STACK_DEPTH)
    std::vector<DevNode> n2(n_nodes);
    std::memcpy(n2.data(), bvh2_nodes, sizeof(DevNode) * n_nodes);
    if (root >= 0 && (uint32_t)root >= n_nodes) return fail(MI355PT_E_INVALID, "root out of range");
    for (const DevNode& n : n2) for (int c = 0; c < 2; ++c) if (n.child[c] >= 0 && (uint32_t)n.child[c] >= n_nodes) return fail(MI355PT_E_INVALID, "child link out of range");
    {   // a cycle or a shared child would make the height computation run forever: every node may be reached once
        std::vector<uint8_t> seen(n_nodes, 0); std::vector<int32_t> st; if (root >= 0) st.push_back(root);
        while (!st.empty()) { const int32_t v = st.back(); st.pop_back(); if (seen[(size_t)v]++) return fail(MI355PT_E_INVALID, "BVH2 is not a tree"); for (int c = 0; c < 2; ++c) if (n2[(size_t)v].child[c] >= 0) st.push_back(n2[(size_t)v].child[c]); }
    }
    std::vector<DevNode4> n4; int32_t root4 = 0; int max_stack = 0; std::string err; const char* method = "";
    if (!collapse_bvh4(n2, root, n_tris, &n4, &root4, &max_stack, &err, &method)) return fail(MI355PT_E_INVALID, err);
    out_info[0] = n_nodes; out_info[1] = (uint32_t)n4.size(); out_info[2] = (uint32_t)(method[0] == 'd' ? 1 : 0); out_info[3] = (uint32_t)max_stack;
    return MI355PT_OK;
}

int mi355pt_probe_bvh_collapse(const float* tri_pos, uint32_t n_tris, const float* rays_od, uint32_t n_rays, uint32_t* out_info, uint32_t* out_mismatch) {
    if (!tri_pos || !out_info || n_tris == 0) return fail(MI355PT_E_INVALID, "bad argument");
    std::vector<BuildTri> bt(n_tris);
    for (uint32_t i = 0; i < n_tris; ++i) for (int a = 0; a < 3; ++a) {
        const float v0 = tri_pos[9 * i + a], v1 = tri_pos[9 * i + 3 + a], v2 = tri_pos[9 * i + 6 + a];
        bt[i].lo[a] = std::fmin(v0, std::fmin(v1, v2)); bt[i].hi[a] = std::fmax(v0, std::fmax(v1, v2)); bt[i].c[a] = 0.5f * (bt[i].lo[a] + bt[i].hi[a]);
    }
    BvhOut bvh; build_bvh(bt, &bvh);
    std::vector<DevNode4> n4; int32_t root4 = 0; int max_stack = 0; std::string err;
    if (!collapse_bvh4(bvh.nodes, bvh.root, bvh.order.size(), &n4, &root4, &max_stack, &err)) return fail(MI355PT_E_INVALID, err);
    out_info[0] = (uint32_t)bvh.nodes.size(); out_info[1] = (uint32_t)n4.size(); out_info[2] = (uint32_t)bvh.max_depth; out_info[3] = (uint32_t)max_stack;
    uint32_t mism = 0;
    auto slab = [](const float lo[3], const float hi[3], const float* o, const float* inv) {
        float tn = 0.0f, tf = 3.0e38f;
        for (int a = 0; a < 3; ++a) { float l = (lo[a] - o[a]) * inv[a], h = (hi[a] - o[a]) * inv[a]; tn = std::fmax(tn, std::fmin(l, h)); tf = std::fmin(tf, std::fmax(l, h)); }
        return tn <= tf;
    };
    for (uint32_t r = 0; rays_od && r < n_rays; ++r) {
        const float* o = rays_od + 6 * r; const float* d = o + 3;
        const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
        std::vector<int32_t> leaves2, leaves4, st;
        st.push_back(bvh.root);
        while (!st.empty()) {
            int32_t c = st.back(); st.pop_back();
            if (c < 0) { leaves2.push_back(c); continue; }
            const DevNode& n = bvh.nodes[(size_t)c];
            for (int k = 0; k < 2; ++k) { float lo[3] = {n.bx[k], n.by[k], n.bz[k]}, hi[3] = {n.bx[2 + k], n.by[2 + k], n.bz[2 + k]}; if (slab(lo, hi, o, inv)) st.push_back(n.child[k]); }
        }
        st.push_back(root4);
        size_t deepest = 0;
        while (!st.empty()) {
            deepest = std::max(deepest, st.size());
            int32_t c = st.back(); st.pop_back();
            if (c < 0) { leaves4.push_back(c); continue; }
            const DevNode4& n = n4[(size_t)c];
            for (int k = 0; k < 4; ++k) { float lo[3] = {n.lox[k], n.loy[k], n.loz[k]}, hi[3] = {n.hix[k], n.hiy[k], n.hiz[k]}; if (slab(lo, hi, o, inv)) st.push_back(n.child[k]); }
        }
        std::sort(leaves2.begin(), leaves2.end()); std::sort(leaves4.begin(), leaves4.end());
        if (leaves2 != leaves4) ++mism;
    }
    if (out_mismatch) *out_mismatch = mism;
    return MI355PT_OK;
}

int mi355pt_scene_export_bvh(const mi355pt_scene* s, void* out_nodes, uint32_t* n_nodes, void* out_tris, uint32_t* n_tris, int32_t* root) {
    if (!s || !n_nodes || !n_tris) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    const DevScene& d = s->impl.dev;
    if (out_nodes) { if (*n_nodes < d.n_nodes) return fail(MI355PT_E_INVALID, "node buffer too small"); if (d.n_nodes) HIP_TRY(hipMemcpy(out_nodes, d.nodes, sizeof(DevNode) * d.n_nodes, hipMemcpyDeviceToHost)); }
    if (out_tris) { if (*n_tris < d.n_tris) return fail(MI355PT_E_INVALID, "triangle buffer too small"); HIP_TRY(hipMemcpy(out_tris, d.tris_render, sizeof(DevTri) * d.n_tris, hipMemcpyDeviceToHost)); }
    *n_nodes = d.n_nodes; *n_tris = d.n_tris;
    if (root) *root = d.root;
    return MI355PT_OK;
}

int mi355pt_render_flow_debug(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, mi355pt_flow_pixel* flow, uint32_t* ids, void* out_hits,
                              mi355pt_stats* stats) {
    if (!out_hits) return fail(MI355PT_E_INVALID, "flow debug: null hit buffer");
    int rc = flow_check(s, cam, p, flow, 1, ids);
    if (rc) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    DevBuf<mi355pt_flow_pixel> d_flow;
    DevBuf<uint32_t> d_ids;
    DevBuf<float4> d_hits;
    HIP_TRY(d_flow.alloc(np));
    HIP_TRY(hipMemset(d_flow.p, 0, np * sizeof(mi355pt_flow_pixel)));
    HIP_TRY(d_ids.alloc_for(ids, np));
    if (ids) HIP_TRY(hipMemset(d_ids.p, 0, np * sizeof(uint32_t)));
    HIP_TRY(d_hits.alloc(np));
    HIP_TRY(hipMemset(d_hits.p, 0, np * sizeof(float4)));
    if ((rc = render_flow_launch(s, cam, p, d_flow.p, d_ids.p, d_hits.p, nullptr, stats))) return rc;
    HIP_TRY(d_flow.download(flow, np));
    HIP_TRY(d_ids.download(ids, np));
    HIP_TRY(d_hits.download((float4*)out_hits, np));
    return MI355PT_OK;
}

int mi355pt_scene_export_flow_mark(const mi355pt_scene* s, void* out_tris, uint32_t* n_tris) {
    if (!s || !n_tris) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (!s->impl.rebase.flow_marked) return fail(MI355PT_E_INVALID, "the scene holds no mark (mi355pt_scene_flow_mark)");
    const uint32_t n = s->impl.dev.n_tris;
    if (out_tris) {
        if (*n_tris < n) return fail(MI355PT_E_INVALID, "triangle buffer too small");
        HIP_TRY(hipDeviceSynchronize());      // the mark's copy is asynchronous on the caller's stream
        if (n) HIP_TRY(hipMemcpy(out_tris, s->impl.rebase.d_tris_prev, sizeof(DevTri) * n, hipMemcpyDeviceToHost));
    }
    *n_tris = n;
    return MI355PT_OK;
}

int mi355pt_scene_export_triangle_ids(const mi355pt_scene* s, uint32_t* out_ids, uint32_t* n_tris) {
    if (!s || !n_tris) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    const uint32_t n = s->impl.dev.n_tris;
    if (out_ids) {
        if (*n_tris < n) return fail(MI355PT_E_INVALID, "id buffer too small");
        std::vector<DevTriShade> shade(n);
        if (n) HIP_TRY(hipMemcpy(shade.data(), s->impl.dev.shade, sizeof(DevTriShade) * n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) { out_ids[2 * (size_t)i] = shade[i].instance; out_ids[2 * (size_t)i + 1] = shade[i].local_tri; }
    }
    *n_tris = n;
    return MI355PT_OK;
}

int mi355pt_probe_intersect(const mi355pt_scene* s, const float* o, const float* d, uint32_t n, float* out_t, uint32_t* out_inst, uint32_t* out_tri,
                            float* out_n) {
    if (!s || !o || !d || !out_t || !out_inst || !out_tri) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (n == 0) return MI355PT_OK;
    DevBuf<float> d_o, d_d, d_t, d_n; DevBuf<uint32_t> d_i, d_tr;
    HIP_TRY(d_o.upload(o, (size_t)n * 3)); HIP_TRY(d_d.upload(d, (size_t)n * 3));
    HIP_TRY(d_t.alloc(n)); HIP_TRY(d_n.alloc((size_t)n * 3)); HIP_TRY(d_i.alloc(n)); HIP_TRY(d_tr.alloc(n));
    HIP_TRY(launch_probe_intersect(s->impl.dev, d_o.p, d_d.p, n, d_t.p, d_i.p, d_tr.p, d_n.p, nullptr));
    HIP_TRY(d_t.download(out_t, n)); HIP_TRY(d_i.download(out_inst, n)); HIP_TRY(d_tr.download(out_tri, n));
    HIP_TRY(d_n.download(out_n, (size_t)n * 3));
    return MI355PT_OK;
}

int mi355pt_probe_occluded(const mi355pt_scene* s, const float* o, const float* d, const float* tmax, uint32_t n, uint8_t* out) {
    if (!s || !o || !d || !tmax || !out) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (n == 0) return MI355PT_OK;
    DevBuf<float> d_o, d_d, d_t; DevBuf<uint8_t> d_out;
    HIP_TRY(d_o.upload(o, (size_t)n * 3)); HIP_TRY(d_d.upload(d, (size_t)n * 3)); HIP_TRY(d_t.upload(tmax, n)); HIP_TRY(d_out.alloc(n));
    HIP_TRY(launch_probe_occluded(s->impl.dev, d_o.p, d_d.p, d_t.p, n, d_out.p, nullptr));
    HIP_TRY(d_out.download(out, n));
    return MI355PT_OK;
}

int mi355pt_probe_sincos(uint32_t first_bits, uint32_t stride, uint32_t n, uint64_t* out_counts) {
    if (!out_counts || stride == 0) return fail(MI355PT_E_INVALID, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MI355PT_E_NO_DEVICE, "no HIP device");
    out_counts[0] = out_counts[1] = out_counts[2] = 0;
    if (n == 0) return MI355PT_OK;
    if ((uint64_t)first_bits + (uint64_t)(n - 1) * stride > 0xffffffffull) return fail(MI355PT_E_INVALID, "bit patterns wrap");
    DevBuf<float> d_s, d_c;
    HIP_TRY(d_s.alloc(n)); HIP_TRY(d_c.alloc(n));
    HIP_TRY(launch_probe_sincos(first_bits, stride, n, d_s.p, d_c.p, nullptr));
    std::vector<float> hs(n), hc(n);
    HIP_TRY(hipMemcpy(hs.data(), d_s.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hc.data(), d_c.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = first_bits + i * stride;
        float x; std::memcpy(&x, &b, 4);
        const float ls = sinf(x), lc = cosf(x);                                   // the libm of this host: what f32::sin / f32::cos call
        out_counts[0]++;
        out_counts[1] += std::memcmp(&ls, &hs[i], 4) != 0 && !(std::isnan(ls) && std::isnan(hs[i]));
        out_counts[2] += std::memcmp(&lc, &hc[i], 4) != 0 && !(std::isnan(lc) && std::isnan(hc[i]));
    }
    return MI355PT_OK;
}

int mi355pt_probe_radiance(const mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_params* p, const uint32_t* xys, uint32_t n, float* out_L,
                           float* out_lambda, float* out_pdf) {
    int rc = check_args(s, cam, p);
    if (rc) return rc;
    if (!xys || !out_L || !out_lambda || !out_pdf) return fail(MI355PT_E_INVALID, "null argument");
    if (n == 0) return MI355PT_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (xys[3 * i] >= cam->width || xys[3 * i + 1] >= cam->height || xys[3 * i + 2] >= p->spp) return fail(MI355PT_E_INVALID, "query outside the frame or the sample range");
    // the whole frame, every sample index, in the launch shape mi355pt_render takes for this job — then pick the queried records
    mi355pt_params q = *p;
    q.shard_index = 0; q.shard_count = 1; q.collect_stats = 0;
    const size_t recs = (size_t)shard_tile_count(cam->width, cam->height, q.shard_index, q.shard_count) * 64u * p->spp;
    if (recs > ((size_t)1 << 26)) return fail(MI355PT_E_INVALID, "frame x spp too large for mi355pt_probe_radiance: use mi355pt_render_sample_log on a sparse shard");
    std::vector<float> L(recs * 4), lam(recs * 4), pdf(recs * 4);
    if ((rc = mi355pt_render_sample_log(s, cam, &q, 0, p->spp, L.data(), lam.data(), pdf.data(), recs, nullptr))) return rc;
    const uint32_t tiles_x = (cam->width + 7) / 8;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = xys[3 * i], y = xys[3 * i + 1], k = xys[3 * i + 2];
        const size_t slot = ((size_t)((y / 8) * tiles_x + x / 8) * 64u + ((y & 7u) * 8u + (x & 7u))) * p->spp + k;
        std::memcpy(out_L + 4 * (size_t)i, &L[4 * slot], 16); std::memcpy(out_lambda + 4 * (size_t)i, &lam[4 * slot], 16);
        std::memcpy(out_pdf + 4 * (size_t)i, &pdf[4 * slot], 16);
    }
    return MI355PT_OK;
}

}  // extern "C"
