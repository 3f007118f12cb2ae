// TEST INFRASTRUCTURE ONLY: array probes over the oracle's own texture and environment-light functions, so that tests/test_lookups.py can pin
// them against the plain NumPy restatements of tests/lookup_reference.py before the GPU is compared with the oracle:
//   bilinear_sample_rgb, sample_normal_map                       (o_spectrum.hpp; texture/sampler.rs:6-45, normal_texture.rs:39-66)
//   EnvLight::build, sample_cdf, sample, direction_pdf, sample_texture   (o_scene.hpp; primitive/impls/environment_light.rs)
// Nothing here restates a lookup: every number returned comes out of the oracle's function.  The one thing the oracle's bilinear lookup does
// not return, the texels it read, is measured from outside: the lookup is bilinear and separable, so its answer on a texture whose column c
// (row r) alone is white is the weight it gave that column (row), and the columns and rows with a non-zero answer are the ones it read.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "o_integrator.hpp"

using namespace oracle;

namespace {

TextureRgb8 make_texture(const uint8_t* rgb, uint32_t w, uint32_t h) {
    TextureRgb8 t; t.w = w; t.h = h; t.data.assign(rgb, rgb + (size_t)w * h * 3);
    return t;
}

struct EnvProbe {
    Rgb2SpecTable table;
    std::vector<float> illuminant;
    EnvLight env;
};

}  // namespace

extern "C" {

// out: n x 3
int lookup_bilinear_rgb(const uint8_t* rgb, uint32_t w, uint32_t h, const float* uv, uint32_t n, float* out) {
    if (!rgb || !uv || !out || w == 0 || h == 0) return -1;
    const TextureRgb8 t = make_texture(rgb, w, h);
    for (uint32_t i = 0; i < n; ++i) bilinear_sample_rgb(t, V2{uv[2 * i], uv[2 * i + 1]}, out + 3 * (size_t)i);
    return 0;
}

// The texels bilinear_sample_rgb reads at each uv of a w x h texture, as the first and last column and the first and last row that carry
// weight: out n x 4 = (x_lo, y_lo, x_hi, y_hi); weights n x 4 = the weights of those two columns and two rows (the same number twice
// where lo == hi).  (w + h) lookups per uv.
int lookup_bilinear_footprint(uint32_t w, uint32_t h, const float* uv, uint32_t n, uint32_t* out, float* weights) {
    if (!uv || !out || !weights || w == 0 || h == 0) return -1;
    std::vector<TextureRgb8> cols(w), rows(h);
    for (uint32_t c = 0; c < w; ++c) {
        cols[c].w = w; cols[c].h = h; cols[c].data.assign((size_t)w * h * 3, 0);
        for (uint32_t y = 0; y < h; ++y) for (int k = 0; k < 3; ++k) cols[c].data[((size_t)y * w + c) * 3 + k] = 255;
    }
    for (uint32_t r = 0; r < h; ++r) {
        rows[r].w = w; rows[r].h = h; rows[r].data.assign((size_t)w * h * 3, 0);
        for (uint32_t x = 0; x < w; ++x) for (int k = 0; k < 3; ++k) rows[r].data[((size_t)r * w + x) * 3 + k] = 255;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const V2 q{uv[2 * i], uv[2 * i + 1]};
        uint32_t lo[2] = {0xffffffffu, 0xffffffffu}, hi[2] = {0, 0};
        float wlo[2] = {0, 0}, whi[2] = {0, 0};
        for (int axis = 0; axis < 2; ++axis) {
            const std::vector<TextureRgb8>& one_hot = axis == 0 ? cols : rows;
            for (uint32_t c = 0; c < (uint32_t)one_hot.size(); ++c) {
                float v[3];
                bilinear_sample_rgb(one_hot[c], q, v);
                if (v[0] != 0.0f) {
                    if (lo[axis] == 0xffffffffu) { lo[axis] = c; wlo[axis] = v[0]; }
                    hi[axis] = c; whi[axis] = v[0];
                }
            }
        }
        uint32_t* o = out + 4 * (size_t)i; float* wt = weights + 4 * (size_t)i;
        o[0] = lo[0]; o[1] = lo[1]; o[2] = hi[0]; o[3] = hi[1];
        wt[0] = wlo[0]; wt[1] = wlo[1]; wt[2] = whi[0]; wt[3] = whi[1];
    }
    return 0;
}

// out: n x 3, the unit tangent-space normal
int lookup_normal_map(const uint8_t* rgb, uint32_t w, uint32_t h, int flip_y, const float* uv, uint32_t n, float* out) {
    if (!rgb || !uv || !out || w == 0 || h == 0) return -1;
    const TextureRgb8 t = make_texture(rgb, w, h);
    for (uint32_t i = 0; i < n; ++i) {
        const V3 v = sample_normal_map(t, flip_y != 0, V2{uv[2 * i], uv[2 * i + 1]});
        out[3 * (size_t)i] = v.x; out[3 * (size_t)i + 1] = v.y; out[3 * (size_t)i + 2] = v.z;
    }
    return 0;
}

// An EnvLight of its own (no scene): rgb h x w x 3, local_to_render as 16 column-major floats, the rgb2spec table and the 470-entry
// illuminant as the scene functions take them.  EnvLight::build has run when this returns.
void* lookup_env_create(const float* table, size_t n_table, const float* illuminant470, const float* rgb, uint32_t w, uint32_t h, const float* l2r) {
    if (!table || !illuminant470 || !rgb || !l2r || w == 0 || h == 0) return nullptr;
    EnvProbe* p = new EnvProbe();
    p->table.data.assign(table, table + n_table);
    if (!p->table.valid()) { delete p; return nullptr; }
    p->illuminant.assign(illuminant470, illuminant470 + NLUT);
    p->env.w = w; p->env.h = h; p->env.rgb.assign(rgb, rgb + (size_t)w * h * 3);
    p->env.illuminant = p->illuminant.data();
    p->env.local_to_render = M4::from_cols16(l2r);
    p->env.build(p->table);
    return p;
}
void lookup_env_destroy(void* handle) { delete (EnvProbe*)handle; }

// marginal: h, conditional: h x w, total_weight: 1
int lookup_env_tables(void* handle, float* marginal, float* conditional, float* total_weight) {
    const EnvLight& e = ((EnvProbe*)handle)->env;
    std::memcpy(marginal, e.marginal.data(), sizeof(float) * e.h);
    std::memcpy(conditional, e.conditional.data(), sizeof(float) * (size_t)e.w * e.h);
    *total_weight = e.total_weight;
    return 0;
}

// dirs: n x 3 render-space directions; out: n
int lookup_env_pdf(void* handle, const float* dirs, uint32_t n, float* out) {
    const EnvLight& e = ((EnvProbe*)handle)->env;
    for (uint32_t i = 0; i < n; ++i) out[i] = e.direction_pdf(V3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]});
    return 0;
}

// u: n x 2.  texel: n x 2 = (x, y), the two sample_cdf calls of EnvLight::sample on their own; wi: n x 3 and pdf: n from EnvLight::sample itself
int lookup_env_sample(void* handle, const float* u, uint32_t n, uint32_t* texel, float* wi, float* pdf) {
    const EnvLight& e = ((EnvProbe*)handle)->env;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t y = EnvLight::sample_cdf(e.marginal.data(), e.h, u[2 * i]);
        const uint32_t x = EnvLight::sample_cdf(&e.conditional[(size_t)y * e.w], e.w, u[2 * i + 1]);
        texel[2 * i] = x; texel[2 * i + 1] = y;
        V3 d; float p;
        e.sample(u[2 * i], u[2 * i + 1], &d, &p);
        wi[3 * i] = d.x; wi[3 * i + 1] = d.y; wi[3 * i + 2] = d.z; pdf[i] = p;
    }
    return 0;
}

// uv: n x 2 texture coordinates; out: n x 3
int lookup_env_sample_texture(void* handle, const float* uv, uint32_t n, float* out) {
    const EnvLight& e = ((EnvProbe*)handle)->env;
    for (uint32_t i = 0; i < n; ++i) e.sample_texture(uv[2 * i], uv[2 * i + 1], out + 3 * (size_t)i);
    return 0;
}

}  // extern "C"
