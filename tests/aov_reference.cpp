// TEST INFRASTRUCTURE ONLY: the CPU restatement of the reference's two AOV renderers, written from
//   renderer/src/renderer/normal_renderer.rs:26-75   (NormalRenderer::render)
//   renderer/src/renderer/albedo_renderer.rs:30-69   (AlbedoRenderer::render)
// on top of the oracle's own Camera, Sampler, Scene::intersect, transforms, spectra and Sensor.  One translation unit that includes the
// oracle's C API, so the library built from it carries the oracle's scene-construction functions under the same `ptoracle_` prefix and
// the tests feed it the scene description they feed the product.  It shares no code with the HIP kernel (csrc/pt_kernels_aov.hip).
#include "oracle_api.cpp"

namespace {

enum { AOV_NORMAL = 0, AOV_ALBEDO = 1, AOV_SHADING_NORMAL = 2 };   // MI355PT_AOV_* (include/mi355pt.h)

// BsdfMaterial::sample_albedo_spectrum (scene/src/material/impls/*.rs)
SS sample_albedo_spectrum(const Scene& scene, const Material& m, V2 uv, const Wavelengths& wl) {
    switch (m.type) {
        case MAT_GLASS:                                                        // glass_material.rs:224-231
        case MAT_PLASTIC: return SS::constant(1.0f);                           // plastic_material.rs:266-273
        case MAT_METAL: return fresnel_complex(1.0f, m.eta.sample(wl), m.k.sample(wl));   // metal_material.rs:267-278
        default: return scene.sample_spectrum_param(m.color, uv, wl, nullptr);  // lambert_material.rs:172-178, simple_pbr*_material.rs: base_color
    }
}

struct PixelClass { uint32_t bsdf = 0, emitter = 0, miss = 0; };

// one pixel, sample indices [s_begin, s_end): the linear sum the renderer divides by spp at its end
V3 render_pixel(const Scene& scene, const Camera& cam, const RenderParams& prm, int kind, const float* illuminant, const float* const cmf[3],
                uint32_t px, uint32_t py, uint32_t s_begin, uint32_t s_end, PixelClass* cls) {
    Sampler smp = Sampler::create((int)prm.sampler, prm.spp, prm.width, prm.height, prm.seed);
    V3 acc{0, 0, 0};
    Sensor sensor; sensor.cmf_x = cmf[0]; sensor.cmf_y = cmf[1]; sensor.cmf_z = cmf[2];
    const float weight = 1.0f;                                                 // FilterSample of the box filter (filter.rs:28)
    for (uint32_t s = s_begin; s < s_end; ++s) {
        smp.start_pixel_sample(px, py, s, prm.width);
        Wavelengths wl = Wavelengths::new_uniform(0.0f);
        if (kind == AOV_ALBEDO) wl = Wavelengths::new_uniform(smp.get_1d());  // albedo_renderer.rs:47-48; the normal renderer draws no wavelength
        const V2 uv = smp.get_2d();                                            // get_2d_pixel
        const Ray ray = cam.sample_ray(px, py, uv);                            // not moved forward
        Intersection hit;
        if (!scene.intersect(ray, std::numeric_limits<float>::max(), &hit, nullptr)) {
            cls->miss++;                                                       // Vec3::ZERO / nothing
            continue;
        }
        const SurfaceInteraction& si = hit.interaction;
        const Material& mat = scene.materials[si.material];
        const bool bsdf = !mat.is_emissive();                                  // as_bsdf_material()
        if (bsdf) cls->bsdf++; else cls->emitter++;
        if (kind == AOV_ALBEDO) {
            if (!bsdf) continue;
            SS sample = sample_albedo_spectrum(scene, mat, si.uv, wl);
            for (int k = 0; k < NS; ++k) sample.v[k] = (sample.v[k] * weight) * Spectrum::lut_value(illuminant, wl.lambda[k]);   // multiply_spectrum
            sensor.add_sample(wl, sample, 1.0f);
        } else {
            V3 n = si.shading_normal;
            if (kind == AOV_NORMAL && bsdf) {
                const M4 render_to_tangent = from_shading_normal_tangent(si.shading_normal, si.tangent);   // shading_transform()
                n = transform_normal(render_to_tangent, si.shading_normal);    // (&render_to_tangent * &interaction).shading_normal
            }
            const V3 color{n.x * 0.5f + 0.5f, n.y * 0.5f + 0.5f, n.z * 0.5f + 0.5f};
            acc = acc + color * weight;
        }
    }
    return kind == AOV_ALBEDO ? sensor.acc : acc;
}

}  // namespace

extern "C" {

// Linear per-pixel sums (W*H*3, added to `accum`) of the 8x8 tiles of the shard in `p`; `classes` (W*H*3 uint32, may be NULL) receives per
// pixel how many of the samples hit a BSDF surface, hit an emitter, missed.  cmf: 3*470 floats as for ptoracle_render_accum.
int ptoracle_render_aov_accum(ptoracle_scene* s, const mi355pt_camera* c, const mi355pt_params* p, int kind, uint32_t illuminant_lut,
                              const float* cmf, uint32_t s_begin, uint32_t s_end, float* accum, uint32_t* classes) {
    if (kind < AOV_NORMAL || kind > AOV_SHADING_NORMAL || s_end > p->spp || s_begin > s_end) return -1;
    if (kind == AOV_ALBEDO && illuminant_lut >= s->scene.luts.size()) return -1;
    const Camera cam = make_camera(c);
    const RenderParams prm = make_params(c, p);
    const float* illuminant = kind == AOV_ALBEDO ? s->scene.luts[illuminant_lut].data() : nullptr;
    const float* const cmfs[3] = {cmf, cmf + NLUT, cmf + 2 * NLUT};
    const uint32_t W = c->width, H = c->height, tiles_x = (W + 7) / 8;
    const uint32_t sc = p->shard_count ? p->shard_count : 1, si = p->shard_count ? p->shard_index : 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            if (((y / 8) * tiles_x + (x / 8)) % sc != si) continue;
            PixelClass cls;
            const V3 a = render_pixel(s->scene, cam, prm, kind, illuminant, cmfs, x, y, s_begin, s_end, &cls);
            float* o = accum + ((size_t)y * W + x) * 3;
            o[0] += a.x; o[1] += a.y; o[2] += a.z;
            if (classes) { uint32_t* q = classes + ((size_t)y * W + x) * 3; q[0] += cls.bsdf; q[1] += cls.emitter; q[2] += cls.miss; }
        }
    return 0;
}

// normal kinds: acc / spp, raw (normal_renderer.rs:71-73).  albedo: Sensor::to_rgb with NoneToneMap and the sRGB OETF (sensor.rs:81-88)
int ptoracle_aov_resolve(int kind, const float* accum, uint32_t n_pixels, uint32_t spp, float* out) {
    for (size_t i = 0; i < (size_t)n_pixels * 3; ++i) {
        float v = accum[i] / (float)spp;
        if (kind == AOV_ALBEDO) v = srgb_oetf(std::fmax(v, 0.0f));
        out[i] = v;
    }
    return 0;
}

}  // extern "C"
