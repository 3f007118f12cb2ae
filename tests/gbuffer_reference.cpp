// TEST INFRASTRUCTURE ONLY: the CPU restatement of the G-buffer pass (include/mi355pt_gbuffer.h, whose comment is the specification) on top
// of the oracle's own Camera, Sampler, Scene::intersect, SurfaceInteraction (position, shading_normal), spectra and Sensor.  One
// translation unit that includes the oracle's C API, so the library built from it carries the oracle's scene-construction functions under
// the same `ptoracle_` prefix and the tests feed it the scene description they feed the product.  It shares no code with the HIP kernel
// (csrc/pt_kernels_gbuffer.hip).
#include "oracle_api.cpp"

namespace {

// BsdfMaterial::sample_albedo_spectrum (scene/src/material/impls/*.rs)
SS gb_albedo_spectrum(const Scene& scene, const Material& m, V2 uv, const Wavelengths& wl) {
    if (m.type == MAT_GLASS || m.type == MAT_PLASTIC) return SS::constant(1.0f);                       // glass_material.rs:224-231, plastic_material.rs:266-273
    if (m.type == MAT_METAL) return fresnel_complex(1.0f, m.eta.sample(wl), m.k.sample(wl));            // metal_material.rs:267-278
    return scene.sample_spectrum_param(m.color, uv, wl, nullptr);                                       // lambert / simple_pbr*: albedo, base_color
}

struct Films { float *albedo, *shading_normal, *position, *hit; };

inline V3 load3(const float* film, size_t o) { return film ? V3{film[o], film[o + 1], film[o + 2]} : V3{0, 0, 0}; }
inline void store3(float* film, size_t o, V3 v) { if (film) { film[o] = v.x; film[o + 1] = v.y; film[o + 2] = v.z; } }

// one pixel, sample indices [s_begin, s_end): every sum starts from the film's value and takes one add per sample, in index order
void gbuffer_pixel(const Scene& scene, const Camera& cam, const RenderParams& prm, const float* illuminant, const float* const cmf[3], uint32_t px,
                   uint32_t py, uint32_t s_begin, uint32_t s_end, const Films& f, size_t o, uint32_t cls[3]) {
    Sampler smp = Sampler::create((int)prm.sampler, prm.spp, prm.width, prm.height, prm.seed);
    Sensor sensor; sensor.cmf_x = cmf[0]; sensor.cmf_y = cmf[1]; sensor.cmf_z = cmf[2];
    sensor.acc = load3(f.albedo, o);
    V3 nrm = load3(f.shading_normal, o), pos = load3(f.position, o), rec = load3(f.hit, o);
    for (uint32_t s = s_begin; s < s_end; ++s) {
        smp.start_pixel_sample(px, py, s, prm.width);
        const Wavelengths wl = Wavelengths::new_uniform(smp.get_1d());          // drawn whichever films are requested
        const V2 uv = smp.get_2d();                                             // get_2d_pixel
        const Ray ray = cam.sample_ray(px, py, uv);                             // not moved forward
        Intersection hit;
        if (!scene.intersect(ray, std::numeric_limits<float>::max(), &hit, nullptr)) { cls[2]++; continue; }   // a miss adds 0 to every film
        const SurfaceInteraction& si = hit.interaction;
        const Material& mat = scene.materials[si.material];
        const bool emitter = mat.is_emissive();
        cls[emitter ? 1 : 0]++;
        if (f.albedo && !emitter) {
            SS a = gb_albedo_spectrum(scene, mat, si.uv, wl);
            for (int k = 0; k < NS; ++k) a.v[k] = (a.v[k] * 1.0f) * Spectrum::lut_value(illuminant, wl.lambda[k]);   // box filter weight 1, times D65
            sensor.add_sample(wl, a, 1.0f);
        }
        const V3 n = si.shading_normal;
        nrm = nrm + V3{n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f};
        pos = pos + si.position;
        rec = rec + V3{hit.t_hit, 1.0f, emitter ? 1.0f : 0.0f};
    }
    store3(f.albedo, o, sensor.acc); store3(f.shading_normal, o, nrm); store3(f.position, o, pos); store3(f.hit, o, rec);
}

}  // namespace

extern "C" {

// Continues the sums of the requested films (W*H*3 floats each, NULL = not wanted) over sample indices [s_begin, s_end) for the 8x8 tiles of
// the shard in `p`; `classes` (W*H*3 uint32, may be NULL) receives per pixel how many of the samples hit a BSDF surface, hit an emitter,
// missed.  cmf: 3*470 floats as for ptoracle_render_accum.  The refusals of mi355pt_render_gbuffer_accum_device return -1.
int ptoracle_render_gbuffer_accum(ptoracle_scene* s, const mi355pt_camera* c, const mi355pt_params* p, uint32_t illuminant_lut, const float* cmf,
                                  uint32_t s_begin, uint32_t s_end, float* albedo, float* shading_normal, float* position, float* hit,
                                  uint32_t* classes) {
    const Films f{albedo, shading_normal, position, hit};
    const float* all[4] = {albedo, shading_normal, position, hit};
    if (!albedo && !shading_normal && !position && !hit) return -1;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (all[i] && all[i] == all[j]) return -1;
    if (s_end > p->spp || s_begin > s_end || c->width == 0 || c->height == 0) return -1;
    if (albedo && illuminant_lut >= s->scene.luts.size()) return -1;
    const Camera cam = make_camera(c);
    const RenderParams prm = make_params(c, p);
    const float* illuminant = albedo ? s->scene.luts[illuminant_lut].data() : nullptr;
    const float* const cmfs[3] = {cmf, cmf + NLUT, cmf + 2 * NLUT};
    const uint32_t W = c->width, H = c->height, tiles_x = (W + 7) / 8;
    const uint32_t sc = p->shard_count ? p->shard_count : 1, si = p->shard_count ? p->shard_index : 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            if (((y / 8) * tiles_x + (x / 8)) % sc != si) continue;
            const size_t o = ((size_t)y * W + x) * 3;
            uint32_t cls[3] = {0, 0, 0};
            gbuffer_pixel(s->scene, cam, prm, illuminant, cmfs, x, y, s_begin, s_end, f, o, cls);
            if (classes) { classes[o] += cls[0]; classes[o + 1] += cls[1]; classes[o + 2] += cls[2]; }
        }
    return 0;
}

}  // extern "C"
