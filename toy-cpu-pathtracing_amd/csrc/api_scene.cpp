// The scene-description part of include/mi355pt.h: create / destroy, the tables, textures, meshes, materials, lights and instances a scene is
// made of, the build, and the two host-only helpers (coat albedo table, u8 quantisation).  Host C++ only; the lowering is scene.cpp's.
#include <cstdio>
#include <cstring>
#include <new>

#include "api_internal.hpp"

using namespace pt;

// The ONE validator of a material descriptor: mi355pt_scene_add_material's and mi355pt_scene_edit's (scene_edit.cpp).  *out: the record of
// the description (the build's finish_materials adds the texture descriptors and the coat table's offset); *err: the refusal's text
int pt::lower_material_desc(const SceneImpl& im, const mi355pt_material_desc& d, DevMaterial* out, std::string* err) {
    auto bad_rc = [&](int code, const std::string& msg) { *err = msg; return code; };
    auto bad = [&](const char* msg) { return bad_rc(MI355PT_E_INVALID, msg); };
    DevMaterial m{};
    int rc;
    m.type = d.type;
    m.normal_tex = d.normal_tex; m.normal_flip_y = d.normal_flip_y; m.thin = d.thin;
    m.intensity = d.intensity; m.roughness = d.roughness; m.metallic = d.metallic; m.ior = d.ior;
    m.cc_ior = d.clearcoat_ior; m.cc_roughness = d.clearcoat_roughness; m.cc_thickness = d.clearcoat_thickness;
    m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu;
    m.intensity_avg = d.intensity;
    if (d.type == MI355PT_MAT_EMISSIVE && d.intensity_tex != MI355PT_NONE) {
        // FloatParameter::texture intensity (emissive_material.rs:55-56,69-76): the device reads it at the hit / sampled uv through the
        // material's metallic_tex slot; the light-pick weight uses ONE value, the texture at uv (0.5, 0.5), computed here with the device's
        // bilinear arithmetic (texture/sampler.rs:81-107: red channel of the gamma-encoded texel / 255)
        if (d.intensity_tex >= im.textures.size()) return bad("bad intensity texture id");
        m.metallic_tex = d.intensity_tex;
        const SceneImpl::Tex& t = im.textures[d.intensity_tex];
        const float u = std::fabs(0.5f - std::trunc(0.5f)), v = 1.0f - std::fabs(0.5f - std::trunc(0.5f));
        const float x = u * ((float)t.w - 1.0f), y = v * ((float)t.h - 1.0f);
        const uint32_t x0 = (uint32_t)std::floor(x), y0 = (uint32_t)std::floor(y), x1 = std::min(x0 + 1u, t.w - 1u), y1 = std::min(y0 + 1u, t.h - 1u);
        const float fx = x - (float)x0, fy = y - (float)y0;
        auto red = [&](uint32_t xx, uint32_t yy) { return (float)t.rgb[((size_t)yy * t.w + xx) * 3] / 255.0f; };
        const float top = red(x0, y0) * (1.0f - fx) + red(x1, y0) * fx, bottom = red(x0, y1) * (1.0f - fx) + red(x1, y1) * fx;
        m.intensity_avg = top * (1.0f - fy) + bottom * fy;
    }
    if (d.type == MI355PT_MAT_CLEARCOAT && d.clearcoat_thickness_tex != MI355PT_NONE) {
        if (d.clearcoat_thickness_tex >= im.textures.size()) return bad("bad clearcoat thickness texture id");
        m.cc_thickness_tex = d.clearcoat_thickness_tex;
    }
    if (d.type == MI355PT_MAT_GLASS || d.type == MI355PT_MAT_PLASTIC) {   // roughness: FloatParameter (glass_material.rs:42, plastic_material.rs:43)
        if (d.roughness_tex != MI355PT_NONE && d.roughness_tex >= im.textures.size()) return bad("bad roughness texture id");
        m.roughness_tex = d.roughness_tex;
    }
    if (d.type == MI355PT_MAT_SIMPLE_PBR || d.type == MI355PT_MAT_CLEARCOAT || d.type == MI355PT_MAT_METAL) {
        if ((d.metallic_tex != MI355PT_NONE && d.metallic_tex >= im.textures.size()) || (d.roughness_tex != MI355PT_NONE && d.roughness_tex >= im.textures.size()))
            return bad("bad metallic/roughness texture id");
        m.metallic_tex = d.type == MI355PT_MAT_METAL ? 0xffffffffu : d.metallic_tex; m.roughness_tex = d.roughness_tex;
    }
    if (d.normal_tex != MI355PT_NONE && d.normal_tex >= im.textures.size()) return bad("bad normal texture id");
    switch (d.type) {
        case MI355PT_MAT_LAMBERT:
            if ((rc = im.lower_spectrum(d.color, &m.color, true, err))) return bad_rc(rc, *err);
            break;
        case MI355PT_MAT_EMISSIVE:
            // SpectrumParameter::Texture radiance (emissive_material.rs:48-79): an sRGB texture of any SpectrumType, looked up at the hit / sampled uv
            if ((rc = im.lower_spectrum(d.color, &m.color, 2, err))) return bad_rc(rc, "emissive radiance: " + *err);
            break;
        case MI355PT_MAT_GLASS:
        case MI355PT_MAT_PLASTIC:
            if ((rc = im.lower_spectrum(d.eta, &m.eta, false, err))) return bad_rc(rc, "eta: " + *err);
            if ((rc = im.lower_spectrum(d.color, &m.color, d.type == MI355PT_MAT_PLASTIC, err))) return bad_rc(rc, *err);
            break;
        case MI355PT_MAT_CLEARCOAT:
            if ((rc = im.lower_spectrum(d.color, &m.color, true, err))) return bad_rc(rc, *err);
            if ((rc = im.lower_spectrum(d.clearcoat_tint, &m.cc_tint, true, err))) return bad_rc(rc, "clearcoat tint: " + *err);
            break;
        case MI355PT_MAT_SIMPLE_PBR:      // SimplePbrMaterial == the clearcoat material's base layer: thickness 0 takes exactly that path
            m.type = MT_CLEARCOAT; m.cc_thickness = 0.0f; m.cc_ior = 1.5f; m.cc_roughness = 0.0f;
            m.cc_tint.kind = SPK_CONSTANT; m.cc_tint.c[0] = 1.0f;
            if ((rc = im.lower_spectrum(d.color, &m.color, true, err))) return bad_rc(rc, *err);
            break;
        case MI355PT_MAT_METAL:
            if ((rc = im.lower_spectrum(d.eta, &m.eta, false, err))) return bad_rc(rc, "eta: " + *err);
            if ((rc = im.lower_spectrum(d.k, &m.cc_tint, false, err))) return bad_rc(rc, "k: " + *err);
            break;
        default:
            return bad("material type not implemented on the device yet");
    }
    *out = m;
    return MI355PT_OK;
}

// ... and of a delta light's: the hidden emissive material that carries the light's spectrum with intensity 1
int pt::lower_light_desc(const SceneImpl& im, const mi355pt_light_desc& d, DevMaterial* hidden, std::string* err) {
    if (d.kind < MI355PT_LIGHT_POINT || d.kind > MI355PT_LIGHT_DIRECTIONAL) { *err = "bad light kind"; return MI355PT_E_INVALID; }
    DevMaterial m{};
    m.type = MT_EMISSIVE; m.normal_tex = 0xffffffffu; m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu; m.intensity = 1.0f; m.intensity_avg = 1.0f;
    std::string why;
    if (int rc = im.lower_spectrum(d.spectrum, &m.color, false, &why)) { *err = "light spectrum: " + why; return rc; }
    *hidden = m;
    return MI355PT_OK;
}

extern "C" {

int mi355pt_scene_create(mi355pt_scene** out) {
    if (!out) return fail(MI355PT_E_INVALID, "null out");
    *out = new (std::nothrow) mi355pt_scene();
    return *out ? MI355PT_OK : fail(MI355PT_E_INVALID, "allocation failed");
}
void mi355pt_scene_destroy(mi355pt_scene* s) { delete s; }

int mi355pt_scene_set_rgb2spec(mi355pt_scene* s, const float* table, size_t n) {
    if (!s || !table || n != (size_t)(64 + 3 * 64 * 64 * 64 * 3)) return fail(MI355PT_E_INVALID, "rgb2spec table must have 64 + 3*64^3*3 floats");
    s->impl.table.assign(table, table + n);
    return MI355PT_OK;
}
int mi355pt_scene_add_lut470(mi355pt_scene* s, const float* v, uint32_t* id) {
    if (!s || !v || !id) return fail(MI355PT_E_INVALID, "null argument");
    s->impl.luts.emplace_back(v, v + 470);
    *id = (uint32_t)s->impl.luts.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_tex_rgb8(mi355pt_scene* s, const uint8_t* rgb, uint32_t w, uint32_t h, uint32_t* id) {
    if (!s || !rgb || !id || w == 0 || h == 0) return fail(MI355PT_E_INVALID, "bad texture");
    SceneImpl::Tex t; t.w = w; t.h = h; t.rgb.assign(rgb, rgb + (size_t)w * h * 3);
    s->impl.textures.push_back(std::move(t));
    *id = (uint32_t)s->impl.textures.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_mesh(mi355pt_scene* s, const float* pos, const float* nrm, const float* uv, const float* tri_tangent, const uint32_t* idx,
                           uint32_t nv, uint32_t nt, uint32_t* out) {
    if (!s || !pos || !nrm || !idx || !out || nv == 0 || nt == 0) return fail(MI355PT_E_INVALID, "bad mesh");
    if ((uv != nullptr) != (tri_tangent != nullptr)) return fail(MI355PT_E_INVALID, "uv and tri_tangent must be given together");
    for (size_t i = 0; i < (size_t)nt * 3; ++i) if (idx[i] >= nv) return fail(MI355PT_E_INVALID, "vertex index out of range");
    // a non-finite position would poison every box above it in the BVH: refuse it here rather than render garbage
    for (size_t i = 0; i < (size_t)nv * 3; ++i) if (!std::isfinite(pos[i])) return fail(MI355PT_E_INVALID, "non-finite vertex position");
    HostMesh m; m.n_vert = nv; m.n_tri = nt;
    m.pos.assign(pos, pos + (size_t)nv * 3);
    m.nrm.resize((size_t)nv * 3);
    for (uint32_t i = 0; i < nv; ++i) {   // Normal::new normalises and Normal::from renormalises (normal.rs:18-20,93-100)
        V3 n = norm3(norm3(V3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}));
        m.nrm[3 * i] = n.x; m.nrm[3 * i + 1] = n.y; m.nrm[3 * i + 2] = n.z;
    }
    if (uv) { m.uv.assign(uv, uv + (size_t)nv * 2); m.tangent.assign(tri_tangent, tri_tangent + (size_t)nt * 3); }
    m.idx.assign(idx, idx + (size_t)nt * 3);
    s->impl.meshes.push_back(std::move(m));
    *out = (uint32_t)s->impl.meshes.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_material(mi355pt_scene* s, const mi355pt_material_desc* d, uint32_t* out) {
    if (!s || !d || !out) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& im = s->impl;
    DevMaterial m{};
    std::string err;
    if (int rc = lower_material_desc(im, *d, &m, &err)) return fail(rc, err);
    im.materials.push_back(m);
    *out = (uint32_t)im.materials.size() - 1;
    return MI355PT_OK;
}
int mi355pt_scene_add_delta_light(mi355pt_scene* s, const mi355pt_light_desc* d) {
    if (!s || !d) return fail(MI355PT_E_INVALID, "null argument");
    SceneImpl& im = s->impl;
    DevMaterial m{};
    std::string err;
    if (int rc = lower_light_desc(im, *d, &m, &err)) return fail(rc, err);
    im.materials.push_back(m);
    HostDeltaLight hl{*d, (uint32_t)im.materials.size() - 1, (uint32_t)im.instances.size()};
    im.delta_lights.push_back(hl);
    return MI355PT_OK;
}
int mi355pt_scene_add_environment_light(mi355pt_scene* s, float intensity, const float* rgb, uint32_t w, uint32_t h, const float* l2w,
                                        uint32_t illuminant_lut) {
    if (!s || !rgb || !l2w || w == 0 || h == 0) return fail(MI355PT_E_INVALID, "bad environment light arguments");
    SceneImpl& im = s->impl;
    if (illuminant_lut >= im.luts.size()) return fail(MI355PT_E_INVALID, "bad illuminant LUT id");
    SceneImpl::HostEnv he;
    he.intensity = intensity; he.w = w; he.h = h; he.illuminant_lut = illuminant_lut;
    he.rgb.assign(rgb, rgb + (size_t)w * h * 3);
    std::memcpy(he.l2w, l2w, sizeof(float) * 16);
    im.envs.push_back(std::move(he));
    DevMaterial m{};                         // hidden emissive material: the integrated RgbIlluminantSpectrum, filled in at build()
    m.type = MT_EMISSIVE; m.normal_tex = 0xffffffffu; m.metallic_tex = m.roughness_tex = m.cc_thickness_tex = 0xffffffffu; m.intensity = 1.0f; m.intensity_avg = 1.0f; m.color.kind = SPK_CONSTANT;
    im.materials.push_back(m);
    mi355pt_light_desc ld{}; ld.kind = LK_ENV; ld.intensity = intensity; std::memcpy(ld.local_to_world, l2w, sizeof(float) * 16);
    im.delta_lights.push_back(HostDeltaLight{ld, (uint32_t)im.materials.size() - 1, (uint32_t)im.instances.size(), (uint32_t)im.envs.size() - 1});
    return MI355PT_OK;
}
int mi355pt_scene_add_instance(mi355pt_scene* s, uint32_t geom, uint32_t mat, const float* l2w) {
    if (!s || !l2w) return fail(MI355PT_E_INVALID, "null argument");
    if (geom >= s->impl.meshes.size() || mat >= s->impl.materials.size()) return fail(MI355PT_E_INVALID, "bad geometry/material id");
    HostInstance hi; hi.geom = geom; hi.mat = mat; std::memcpy(hi.l2w, l2w, sizeof(float) * 16);
    s->impl.instances.push_back(hi);
    return MI355PT_OK;
}
int mi355pt_coat_albedo_table(float alpha, float r0, float* out) {
    if (!out || !(alpha >= 0.0f) || !(r0 >= 0.0f)) return fail(MI355PT_E_INVALID, "bad argument");
    coat_albedo_table(alpha, r0, out);
    return MI355PT_OK;
}
int mi355pt_scene_set_bvh_builder(mi355pt_scene* s, int mode) {
    if (!s) return fail(MI355PT_E_INVALID, "null argument");
    if (mode != MI355PT_BVH_AUTO && mode != MI355PT_BVH_HOST && mode != MI355PT_BVH_GPU) return fail(MI355PT_E_INVALID, "unknown BVH builder mode");
    s->impl.bvh_builder = mode;
    return MI355PT_OK;
}
int mi355pt_scene_build(mi355pt_scene* s, const mi355pt_camera* cam) {
    if (!s || !cam) return fail(MI355PT_E_INVALID, "null argument");
    std::string err;
    float cmf[470 * 4];
    cie_cmf4(cmf);
    int rc = s->impl.build(cam, cmf, &err);
    // the launch context belongs to the old build: another feature set launches other kernels (cached grid sizes), another device makes its
    // buffers foreign memory — get_launch_ctx makes a new one, on the build's device, at the next render
    delete s->ctx; s->ctx = nullptr;
    return rc ? fail(rc, err) : MI355PT_OK;
}

int mi355pt_scene_info(const mi355pt_scene* s, char* buf, size_t n) {
    if (!s || !buf || n == 0) return fail(MI355PT_E_INVALID, "null argument");
    if (!s->impl.built) return fail(MI355PT_E_INVALID, "scene not built");
    std::snprintf(buf, n, "%s", s->impl.info.c_str());
    return MI355PT_OK;
}

int mi355pt_quantize_u8(const float* rgb, size_t n, uint8_t* out) {
    if (!rgb || !out) return fail(MI355PT_E_INVALID, "null argument");
    for (size_t i = 0; i < n; ++i) {   // Rust `as u8`: saturating, NaN -> 0 (renderer.rs:141-143)
        float v = rgb[i] * 255.0f;
        out[i] = std::isnan(v) ? 0 : (v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (uint8_t)v));
    }
    return MI355PT_OK;
}

}  // extern "C"
