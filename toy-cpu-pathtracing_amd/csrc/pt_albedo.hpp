// BsdfMaterial::sample_albedo_spectrum on the device, shared by the two primary-ray units that write an albedo film: the AOV kernel
// (pt_kernels_aov.hip) and the G-buffer kernel (pt_kernels_gbuffer.hip).  One definition, so the two films cannot drift apart.
#pragma once
#include "pt_kernel.hpp"

namespace pt {

// sample_albedo_spectrum (lambert_material.rs:172-178, simple_pbr_material.rs:259-266, simple_pbr_clearcoat_material.rs:435-442: the
// albedo / base colour parameter; glass_material.rs:224-231, plastic_material.rs:266-273: 1; metal_material.rs:267-278:
// fresnel_complex(1.0, eta, k))
template <uint32_t FEAT>
PT_DEV void albedo_spectrum(const DevScene& sc, const DevMaterial* mat, const Wl& wl, f2 uv, float out[4], StatCounters& st) {
    const uint32_t mtype = mat->type;
    if (mtype == MT_GLASS || mtype == MT_PLASTIC) {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = 1.0f;
    } else if (mtype == MT_METAL) {
        float eta[4], k[4];
        const DevSpectrum es = load_spectrum(&mat->eta), ks = load_spectrum(&mat->cc_tint);   // (the metal's k lives in cc_tint, layout.hpp)
        eval_spectrum<false, false>(sc, es, wl, uv, eta, st);
        eval_spectrum<false, false>(sc, ks, wl, uv, k, st);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = fresnel_complex1(1.0f, eta[i], k[i]);
    } else {
        const DevSpectrum cs = load_spectrum(&mat->color);
        eval_spectrum<false, (FEAT & FEAT_TEX) != 0u>(sc, cs, wl, uv, out, st);
    }
}

}  // namespace pt
