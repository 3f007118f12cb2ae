// Editing lights and materials of a built scene (include/mi355pt_edit.h): the call itself and its host-only twin of the debug surface.
// Host C++ only; the device half is scene_update.cpp's step, the kernel is pt_kernels_edit.hip, what the host decides before the step is
// scene_edit_plan.hpp.  The records are the lowering's own (scene_lower.cpp lower_edit_records), the descriptors go through the add calls'
// validators (api_scene.cpp); the host form the tests hold the edit to is mi355pt_scene_debug_pinned_digest (scene_debug.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355pt_debug.h"
#include "scene_edit_plan.hpp"
#include "scene_update.hpp"

using namespace pt;

static_assert(EDIT_MT_EMISSIVE == MT_EMISSIVE && EDIT_MT_CLEARCOAT == MT_CLEARCOAT && EDIT_SPK_TEXTURE == SPK_TEXTURE, "scene_edit_plan.hpp restates layout.hpp");
static_assert(EDIT_IN_PLACE == MI355PT_MOVE_REBASED && EDIT_UNSUPPORTED_BUILD == MI355PT_MOVE_UNSUPPORTED_BUILD && EDIT_SAME_RECORDS == MI355PT_EDIT_SAME_RECORDS &&
              EDIT_EMITTER_SET_CHANGED == MI355PT_EDIT_EMITTER_SET_CHANGED && EDIT_TABLE_SHAPE_CHANGED == MI355PT_EDIT_TABLE_SHAPE_CHANGED, "scene_edit_plan.hpp restates the headers");
static_assert(MI355PT_EDIT_SAME_RECORDS == MI355PT_MOVE_SAME_VERTICES + 1, "the reasons continue mi355pt_deform.h's");

namespace {

// the edits, checked: the records as the description will hold them
struct Checked {
    struct Material { uint32_t mat; DevMaterial rec; };
    struct Light { uint32_t slot; mi355pt_light_desc desc; DevMaterial hidden; };   // slot: index in SceneImpl::delta_lights
    struct Env { uint32_t slot, env; float intensity; const float* l2w; const float* rgb; };
    std::vector<Material> materials;
    std::vector<Light> lights;
    std::vector<Env> envs;
};

bool spectrum_finite(const DevSpectrum& sp) {
    if (sp.kind == SPK_CONSTANT) return std::isfinite(sp.c[0]);
    if (sp.kind == SPK_SIGMOID) return std::isfinite(sp.c[0]) && std::isfinite(sp.c[1]) && std::isfinite(sp.c[2]);
    return true;
}
// a texture or LUT the record names that the build did not upload
bool names_later_table(const DevMaterial& m, size_t n_textures, size_t n_luts) {
    for (uint32_t t : {m.normal_tex, m.metallic_tex, m.roughness_tex, m.cc_thickness_tex}) if (t != 0xffffffffu && t >= n_textures) return true;
    for (const DevSpectrum* sp : {&m.color, &m.eta, &m.cc_tint}) {
        if (sp->kind == SPK_LUT && sp->id >= n_luts) return true;
        if (sp->kind != SPK_TEXTURE) continue;
        uint32_t sub, lut;
        std::memcpy(&sub, &sp->c[0], 4); std::memcpy(&lut, &sp->c[1], 4);
        if (sp->id >= n_textures || (sub == 1u && lut >= n_luts)) return true;
    }
    return false;
}
// finite, and a linear part that inverts (lower_delta_light and lower_environment invert it)
const char* matrix_fault(const float* m) {
    for (int k = 0; k < 16; ++k) if (!std::isfinite(m[k])) return "non-finite";
    const double a[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    const double det = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[3] * (a[1] * a[8] - a[7] * a[2]) + a[6] * (a[1] * a[5] - a[4] * a[2]);
    return det == 0.0 || !std::isfinite(det) ? "singular" : nullptr;
}

// every check of the edits that needs no device and no built scene; *err names the first one that fails
bool check_edits(const SceneImpl& impl, const mi355pt_scene_edits& e, Checked* out, std::string* err) {
    *out = Checked{};
    // textures and LUTs: the build's (or the pin's); a scene that is neither built nor pinned has the description's
    const size_t n_textures = impl.rebase.pinned ? impl.rebase.textures.size() : impl.textures.size();
    const size_t n_luts = impl.rebase.pinned ? (size_t)impl.rebase.n_luts : impl.luts.size();
    std::vector<uint8_t> hidden(impl.materials.size(), 0);
    std::vector<uint32_t> delta_slot, env_slot(impl.envs.size(), 0u);       // creation order -> index in delta_lights
    for (size_t k = 0; k < impl.delta_lights.size(); ++k) {
        const HostDeltaLight& hl = impl.delta_lights[k];
        hidden[hl.material] = 1;
        if (hl.d.kind == LK_ENV) env_slot[hl.env_index] = (uint32_t)k; else delta_slot.push_back((uint32_t)k);
    }
    for (uint32_t k = 0; k < e.n_materials; ++k) {
        const mi355pt_material_edit& me = e.materials[k];
        if (me.mat >= impl.materials.size() || hidden[me.mat]) { *err = "bad material id"; return false; }
        if (k && me.mat <= e.materials[k - 1].mat) { *err = "material ids must be strictly ascending"; return false; }
        Checked::Material c{me.mat, DevMaterial{}};
        if (lower_material_desc(impl, me.desc, &c.rec, err)) return false;
        if (names_later_table(c.rec, n_textures, n_luts)) { *err = "a texture or LUT id that did not exist at the build"; return false; }
        const DevMaterial& m = c.rec;
        for (float v : {m.intensity, m.roughness, m.metallic, m.ior, m.cc_ior, m.cc_roughness, m.cc_thickness, m.intensity_avg})
            if (!std::isfinite(v)) { *err = "non-finite material parameter"; return false; }
        if (!spectrum_finite(m.color) || !spectrum_finite(m.eta) || !spectrum_finite(m.cc_tint)) { *err = "non-finite material parameter"; return false; }
        out->materials.push_back(c);
    }
    for (uint32_t k = 0; k < e.n_lights; ++k) {
        const mi355pt_light_edit& le = e.lights[k];
        if (le.light >= delta_slot.size()) { *err = "bad light id"; return false; }
        if (k && le.light <= e.lights[k - 1].light) { *err = "light ids must be strictly ascending"; return false; }
        Checked::Light c{delta_slot[le.light], le.desc, DevMaterial{}};
        if (lower_light_desc(impl, le.desc, &c.hidden, err)) return false;
        if (names_later_table(c.hidden, n_textures, n_luts)) { *err = "a texture or LUT id that did not exist at the build"; return false; }
        if (!std::isfinite(le.desc.intensity) || !std::isfinite(le.desc.angle_inner) || !std::isfinite(le.desc.angle_outer) || !spectrum_finite(c.hidden.color)) { *err = "non-finite light parameter"; return false; }
        if (const char* fault = matrix_fault(le.desc.local_to_world)) { *err = std::string(fault) + " light transform"; return false; }
        out->lights.push_back(c);
    }
    for (uint32_t k = 0; k < e.n_envs; ++k) {
        const mi355pt_env_edit& ee = e.envs[k];
        if (ee.env >= impl.envs.size()) { *err = "bad environment light id"; return false; }
        if (k && ee.env <= e.envs[k - 1].env) { *err = "environment light ids must be strictly ascending"; return false; }
        if (!std::isfinite(ee.intensity)) { *err = "non-finite light parameter"; return false; }
        if (ee.local_to_world) if (const char* fault = matrix_fault(ee.local_to_world)) { *err = std::string(fault) + " light transform"; return false; }
        const SceneImpl::HostEnv& he = impl.envs[ee.env];
        if (ee.rgb) for (size_t i = 0; i < (size_t)he.w * he.h * 3; ++i) if (!std::isfinite(ee.rgb[i])) { *err = "non-finite environment map value"; return false; }
        out->envs.push_back(Checked::Env{env_slot[ee.env], ee.env, ee.intensity, ee.local_to_world, ee.rgb});
    }
    return true;
}

bool null_edits(const mi355pt_scene_edits* e) {
    return !e || (e->n_materials == 0 && e->n_lights == 0 && e->n_envs == 0) || (e->n_materials && !e->materials) || (e->n_lights && !e->lights) || (e->n_envs && !e->envs);
}

// the description takes the edited records.  *material_changed (per material) and *env_map_changed (per environment), NULL ok: which
// records and which maps differ bytewise from what the description held
void apply_edits(SceneImpl* impl, const Checked& c, std::vector<uint8_t>* material_changed, std::vector<uint8_t>* env_map_changed) {
    if (material_changed) material_changed->assign(impl->materials.size(), 0);
    if (env_map_changed) env_map_changed->assign(impl->envs.size(), 0);
    auto set_material = [&](uint32_t mat, const DevMaterial& rec) {
        if (material_changed && !edit_same_bytes(&rec, &impl->materials[mat], sizeof(DevMaterial))) (*material_changed)[mat] = 1;
        impl->materials[mat] = rec;
    };
    for (const Checked::Material& m : c.materials) set_material(m.mat, m.rec);
    for (const Checked::Light& l : c.lights) {
        HostDeltaLight& hl = impl->delta_lights[l.slot];
        hl.d = l.desc;
        set_material(hl.material, l.hidden);
    }
    for (const Checked::Env& ev : c.envs) {
        SceneImpl::HostEnv& he = impl->envs[ev.env];
        HostDeltaLight& hl = impl->delta_lights[ev.slot];
        he.intensity = ev.intensity; hl.d.intensity = ev.intensity;
        if (ev.l2w) { std::memcpy(he.l2w, ev.l2w, sizeof(he.l2w)); std::memcpy(hl.d.local_to_world, ev.l2w, sizeof(he.l2w)); }
        if (ev.rgb) {
            if (env_map_changed && !edit_same_bytes(ev.rgb, he.rgb.data(), he.rgb.size() * sizeof(float))) (*env_map_changed)[ev.env] = 1;
            he.rgb.assign(ev.rgb, ev.rgb + he.rgb.size());
        }
    }
}

}  // namespace

extern "C" {

int mi355pt_scene_edit(mi355pt_scene* s, const mi355pt_camera* cam, const mi355pt_scene_edits* e, mi355pt_edit_result* out) {
    const auto t0 = std::chrono::steady_clock::now();
    mi355pt_edit_result r{};
    if (out) *out = r;
    if (!s || !cam || null_edits(e)) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& impl = s->impl;
    Checked edits;
    std::string err;
    if (!check_edits(impl, *e, &edits, &err)) return fail(MI355PT_E_INVALID, err);
    if (!s->parts.empty()) return fail(MI355PT_E_INVALID, "mi355pt_scene_edit does not edit a scene built with mi355pt_scene_build_multi: build it again");
    if (!impl.built) return fail(MI355PT_E_NOT_BUILT, "scene not built");
    if (std::memcmp(cam->position, impl.build_cam_pos, sizeof(float) * 3) != 0) return fail(MI355PT_E_INVALID, "camera position differs from the position the scene is at: call mi355pt_scene_move_camera first");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != impl.device) return fail(MI355PT_E_DEVICE, "current HIP device is not the device the scene was built on");
    r.features_before = r.features_after = impl.features;
    auto done = [&](int rc) { r.host_ms = ms_since(t0); if (out) *out = r; return rc; };

    // the description takes the edited records now: everything below — the records, the checks, a rebuild — is computed from it
    std::vector<EditMaterialKey> before, after;
    material_keys(impl.materials, &before);
    std::vector<uint8_t> material_changed, env_map_changed, env_edited(impl.envs.size(), 0);
    // what the edits replace, kept until the records are lowered: an edit that cannot be lowered leaves the description as it was
    const std::vector<DevMaterial> old_materials = impl.materials;
    const std::vector<HostDeltaLight> old_lights = impl.delta_lights;
    std::vector<SceneImpl::HostEnv> old_envs;
    for (const Checked::Env& ev : edits.envs) old_envs.push_back(impl.envs[ev.env]);
    apply_edits(&impl, edits, &material_changed, &env_map_changed);
    material_keys(impl.materials, &after);
    for (const Checked::Env& ev : edits.envs) env_edited[ev.env] = 1;
    auto rebuild = [&](uint32_t reason) {
        r.rebuilt = 1; r.reason = reason; r.launches = 0; r.device_ms = 0.0;
        const int rc = mi355pt_scene_build(s, cam);
        if (rc == MI355PT_OK) r.features_after = impl.features;
        return done(rc);
    };
    RebaseState& rb = impl.rebase;
    if (const uint32_t reason = edit_fallback_reason(before.data(), after.data(), after.size(), rb.ready)) return rebuild(reason);

    // host: the records with the lowering's own functions, then what of them differs from the built ones
    EditRecords rec;
    if (int rc = lower_edit_records(impl, cam, rb, material_changed.data(), env_edited.data(), &rec, &err)) {
        impl.materials = old_materials; impl.delta_lights = old_lights;
        for (size_t k = 0; k < edits.envs.size(); ++k) impl.envs[edits.envs[k].env] = std::move(old_envs[k]);
        return done(fail(rc, err));
    }
    const bool same_materials = edit_same_bytes(rec.materials, rb.materials), same_cc = edit_same_bytes(rec.cc_albedo, rb.cc_albedo);
    const bool same_lights = edit_same_bytes(rec.lights, rb.lights), same_envs = edit_same_bytes(rec.envs, rb.envs);
    bool same_maps = true;
    for (uint8_t c : env_map_changed) if (c) same_maps = false;
    if (same_materials && same_cc && same_lights && same_envs && same_maps) { r.reason = MI355PT_EDIT_SAME_RECORDS; return done(MI355PT_OK); }
    std::vector<EditMaterialKey> built_keys, new_keys;
    material_keys(rb.materials, &built_keys); material_keys(rec.materials, &new_keys);
    uint32_t n_reclassed = 0;
    const std::vector<uint32_t> class_table = edit_class_table(built_keys.data(), new_keys.data(), new_keys.size(), &n_reclassed);

    // from here on the device: a HIP error drops the scene, since the description already holds the edited records
    EditStage stage;
    if (!same_materials) stage.materials = &rec.materials;
    if (!same_cc) stage.cc_albedo = &rec.cc_albedo;
    if (!same_lights) stage.lights = &rec.lights;
    if (!same_envs || !same_maps) { stage.envs = &rec.envs; stage.env_tables = &rec.env_tables; stage.env_map_changed = env_map_changed.data(); }
    if (n_reclassed) stage.class_table = &class_table;
    const CameraRecords none;
    SceneUpdate update{none, false};
    update.edit = &stage;
    const SceneUpdateResult res = scene_update_step(&impl, update);
    r.launches = res.launches; r.device_ms = res.device_ms;
    if (res.outcome != SceneUpdateResult::DONE) return done(fail(MI355PT_E_DEVICE, res.what));

    // the caches the next update starts from, and the feature set the next render selects its kernel from
    rb.materials = std::move(rec.materials); rb.cc_albedo = std::move(rec.cc_albedo); rb.lights = std::move(rec.lights); rb.envs = std::move(rec.envs);
    if (rec.features != impl.features) {
        impl.features = rec.features;
        const size_t at = impl.info.rfind(" features=");
        if (at != std::string::npos) impl.info = impl.info.substr(0, at) + " features=" + std::to_string(rec.features);
        if (s->ctx) {                                                         // the resident waves cached per kernel of the OLD feature set
            std::memset(s->ctx->waves, 0, sizeof(s->ctx->waves)); std::memset(s->ctx->aov_waves, 0, sizeof(s->ctx->aov_waves)); s->ctx->gbuffer_waves = 0;
        }
    }
    r.features_after = impl.features;
    r.reason = MI355PT_MOVE_REBASED;
    return done(MI355PT_OK);
}

int mi355pt_scene_debug_apply_edits(mi355pt_scene* s, const mi355pt_scene_edits* e) {
    if (!s || null_edits(e)) return fail(MI355PT_E_INVALID, "null argument");
    if (s->impl.built || !s->parts.empty()) return fail(MI355PT_E_INVALID, "a built scene is edited with mi355pt_scene_edit");
    Checked edits;
    std::string err;
    if (!check_edits(s->impl, *e, &edits, &err)) return fail(MI355PT_E_INVALID, err);
    apply_edits(&s->impl, edits, nullptr, nullptr);
    return MI355PT_OK;
}

}  // extern "C"
