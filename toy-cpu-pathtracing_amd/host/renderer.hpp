// C++ host side above the C ABI: mirrors the reference's Rust API for the hot path so that scene files and a
// main() read like the reference's (the reference is Rust; no Rust toolchain exists in this image — DESIGN.md §1).
//
//   reference (Rust)                                             here (C++)
//   scene::Scene / create_scene!()   scene/src/scene.rs:36-76    renderer::Scene
//   Scene::load_obj                  scene.rs:47-49              Scene::load_obj   (tobj single_index + triangulate semantics)
//   Scene::create_primitive          scene.rs:57-61              Scene::create_primitive(GeometryPrimitive{..})
//   Scene::build(&camera)            scene.rs:64-76              Scene::build(camera)
//   LambertMaterial::new ...         material/impls/*.rs         LambertMaterial::create ... (value types, no Arc)
//   SpectrumParameter / NormalParameter / FloatParameter         same names
//   RgbTexture::load_srgb, NormalTexture::load                   same names (8-bit binary PPM "P6" files instead of PNG)
//   presets::cie_illum_d6500(), glass_sf11_eta()                 presets::... (baked 470-entry LUTs, data/presets470.bin)
//   Camera::new + set_look_to        renderer/src/camera.rs      renderer::Camera
//   RendererArgs, SrgbRenderer{Pt,Nee,Mis}, RendererImage        same names; RendererImage::render(sampler) calls mi355pt_render
//   RendererImage::save              renderer.rs:137-148         same truncating quantisation, PNG written without zlib
//
// Error behaviour: the reference panics; this layer throws std::runtime_error carrying mi355pt_last_error().
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mi355pt.h"

namespace renderer {

inline void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + mi355pt_last_error());
}

struct Vec3 { float x, y, z; };

// ------------------------------------------------------------------ data directory
inline std::string data_dir() {
    const char* e = std::getenv("MI355PT_DATA");
    return e ? e : "toy-cpu-pathtracing_amd/data";
}

// ------------------------------------------------------------------ spectra
struct Spectrum { mi355pt_spectrum s{}; std::vector<float> lut; };   // lut non-empty => registered lazily per scene

struct ColorSrgb { float r, g, b; };
struct ColorSrgbLinear { float r, g, b; };
struct RgbAlbedoSpectrum {                                            // spectrum/src/spectrum/rgb_albedo_spectrum.rs:21-27
    static Spectrum create(ColorSrgb c) { Spectrum s; s.s.kind = MI355PT_SPEC_RGB_ALBEDO_SRGB; s.s.c[0] = c.r; s.s.c[1] = c.g; s.s.c[2] = c.b; return s; }
    static Spectrum create(ColorSrgbLinear c) { Spectrum s; s.s.kind = MI355PT_SPEC_RGB_ALBEDO_SRGB_LINEAR; s.s.c[0] = c.r; s.s.c[1] = c.g; s.s.c[2] = c.b; return s; }
};
struct ConstantSpectrum {
    static Spectrum create(float v) { Spectrum s; s.s.kind = MI355PT_SPEC_CONSTANT; s.s.c[0] = v; return s; }
};
namespace presets {
inline Spectrum load(const std::string& name) {
    std::ifstream js(data_dir() + "/presets470.json");
    if (!js) throw std::runtime_error("presets470.json not found under " + data_dir());
    std::stringstream ss; ss << js.rdbuf();
    std::string txt = ss.str();
    // names are listed in file order inside "names": [...]
    std::vector<std::string> names;
    size_t lb = txt.find('[', txt.find("\"names\""));
    size_t rb = txt.find(']', lb);
    for (size_t pos = lb;;) {
        size_t q0 = txt.find('"', pos);
        if (q0 == std::string::npos || q0 > rb) break;
        size_t q1 = txt.find('"', q0 + 1);
        names.push_back(txt.substr(q0 + 1, q1 - q0 - 1));
        pos = q1 + 1;
    }
    for (size_t i = 0; i < names.size(); ++i)
        if (names[i] == name) {
            std::ifstream bin(data_dir() + "/presets470.bin", std::ios::binary);
            bin.seekg((std::streamoff)(i * 470 * sizeof(float)));
            Spectrum s; s.s.kind = MI355PT_SPEC_LUT470; s.lut.resize(470);
            bin.read((char*)s.lut.data(), 470 * sizeof(float));
            if (!bin) throw std::runtime_error("presets470.bin truncated");
            return s;
        }
    throw std::runtime_error("unknown preset spectrum " + name);
}
inline Spectrum cie_illum_d6500() { return load("cie_illum_d6500"); }   // spectrum/src/presets.rs:310-312
inline Spectrum glass_sf11_eta() { return load("glass_sf11_eta"); }     // :458-460
inline Spectrum glass_bk7_eta() { return load("glass_bk7_eta"); }
inline Spectrum au_eta() { return load("au_eta"); }  inline Spectrum au_k() { return load("au_k"); }          // metals: presets.rs
inline Spectrum ag_eta() { return load("ag_eta"); }  inline Spectrum ag_k() { return load("ag_k"); }
inline Spectrum cu_eta() { return load("cu_eta"); }  inline Spectrum cu_k() { return load("cu_k"); }
inline Spectrum al_eta() { return load("al_eta"); }  inline Spectrum al_k() { return load("al_k"); }
inline Spectrum cu_zn_eta() { return load("cu_zn_eta"); }  inline Spectrum cu_zn_k() { return load("cu_zn_k"); }
}  // namespace presets

// ------------------------------------------------------------------ textures (scene/src/texture/*.rs)
struct ImageRgb8 { std::vector<uint8_t> rgb; uint32_t w = 0, h = 0; };
inline ImageRgb8 load_ppm(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open texture " + path);
    std::string magic; f >> magic;
    if (magic != "P6") throw std::runtime_error(path + ": expected a binary PPM (P6)");
    auto skip = [&]() { while (true) { int c = f.peek(); if (c == '#') { std::string l; std::getline(f, l); } else if (isspace(c)) f.get(); else break; } };
    ImageRgb8 im; int maxv;
    skip(); f >> im.w; skip(); f >> im.h; skip(); f >> maxv; f.get();
    if (maxv != 255) throw std::runtime_error(path + ": only 8-bit PPM supported");
    im.rgb.resize((size_t)im.w * im.h * 3);
    f.read((char*)im.rgb.data(), (std::streamsize)im.rgb.size());
    if (!f) throw std::runtime_error(path + ": truncated");
    return im;
}
// ---- PNG decoding (the reference's texture/loader.rs:44-64 goes through image::open(..).to_rgb8()): 8- and 16-bit,
// grey / grey+alpha / RGB / RGBA / palette, non-interlaced, own inflate (RFC 1950/1951) so the host mirror needs no libpng/zlib.
namespace png_detail {
struct BitReader {
    const uint8_t* p; size_t n, pos = 0; uint32_t bitbuf = 0; int bitcnt = 0;
    uint32_t bits(int c) {
        while (bitcnt < c) { if (pos >= n) throw std::runtime_error("png: truncated deflate stream"); bitbuf |= (uint32_t)p[pos++] << bitcnt; bitcnt += 8; }
        uint32_t v = c ? (bitbuf & ((1u << c) - 1u)) : 0u; bitbuf >>= c; bitcnt -= c; return v;
    }
    void align() { bitbuf = 0; bitcnt = 0; }
};
struct Huffman {
    uint16_t count[16] = {0}; std::vector<uint16_t> symbol;
    void build(const uint8_t* len, int n) {
        symbol.assign(n, 0);
        for (int i = 0; i < 16; ++i) count[i] = 0;
        for (int i = 0; i < n; ++i) count[len[i]]++;
        count[0] = 0;
        uint16_t offs[16]; offs[1] = 0;
        for (int i = 1; i < 15; ++i) offs[i + 1] = offs[i] + count[i];
        for (int i = 0; i < n; ++i) if (len[i]) symbol[offs[len[i]]++] = (uint16_t)i;
    }
    int decode(BitReader& br) const {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l <= 15; ++l) {
            code |= (int)br.bits(1);
            int c = count[l];
            if (code - c < first) return symbol[index + (code - first)];
            index += c; first += c; first <<= 1; code <<= 1;
        }
        throw std::runtime_error("png: bad Huffman code");
    }
};
inline std::vector<uint8_t> inflate(const uint8_t* data, size_t n) {
    if (n < 6) throw std::runtime_error("png: zlib stream too short");
    BitReader br{data + 2, n - 2};   // skip CMF/FLG
    std::vector<uint8_t> out;
    static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint16_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint16_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    for (bool last = false; !last;) {
        last = br.bits(1) != 0;
        uint32_t type = br.bits(2);
        if (type == 0) {
            br.align();
            if (br.pos + 4 > br.n) throw std::runtime_error("png: truncated stored block");
            uint32_t len = br.p[br.pos] | (br.p[br.pos + 1] << 8); br.pos += 4;
            if (br.pos + len > br.n) throw std::runtime_error("png: truncated stored block");
            out.insert(out.end(), br.p + br.pos, br.p + br.pos + len); br.pos += len;
            continue;
        }
        if (type == 3) throw std::runtime_error("png: bad deflate block type");
        Huffman lit, dist;
        if (type == 1) {
            uint8_t l[320]; int i = 0;
            for (; i < 144; ++i) l[i] = 8;
            for (; i < 256; ++i) l[i] = 9;
            for (; i < 280; ++i) l[i] = 7;
            for (; i < 288; ++i) l[i] = 8;
            lit.build(l, 288);
            for (i = 0; i < 30; ++i) l[i] = 5;
            dist.build(l, 30);
        } else {
            int nlen = (int)br.bits(5) + 257, ndist = (int)br.bits(5) + 1, ncode = (int)br.bits(4) + 4;
            static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t l[320] = {0};
            for (int i = 0; i < ncode; ++i) l[order[i]] = (uint8_t)br.bits(3);
            Huffman cl; cl.build(l, 19);
            uint8_t lens[320] = {0};
            for (int i = 0; i < nlen + ndist;) {
                int sym = cl.decode(br);
                if (sym < 16) lens[i++] = (uint8_t)sym;
                else {
                    int rep; uint8_t v = 0;
                    if (sym == 16) { if (i == 0) throw std::runtime_error("png: bad code lengths"); v = lens[i - 1]; rep = 3 + (int)br.bits(2); }
                    else if (sym == 17) rep = 3 + (int)br.bits(3);
                    else rep = 11 + (int)br.bits(7);
                    if (i + rep > nlen + ndist) throw std::runtime_error("png: bad code lengths");
                    while (rep--) lens[i++] = v;
                }
            }
            lit.build(lens, nlen); dist.build(lens + nlen, ndist);
        }
        for (;;) {
            int sym = lit.decode(br);
            if (sym < 256) out.push_back((uint8_t)sym);
            else if (sym == 256) break;
            else {
                sym -= 257;
                if (sym >= 29) throw std::runtime_error("png: bad length symbol");
                uint32_t len = lbase[sym] + br.bits(lext[sym]);
                int ds = dist.decode(br);
                if (ds >= 30) throw std::runtime_error("png: bad distance symbol");
                uint32_t d = dbase[ds] + br.bits(dext[ds]);
                if (d > out.size()) throw std::runtime_error("png: distance too far back");
                size_t from = out.size() - d;
                for (uint32_t k = 0; k < len; ++k) out.push_back(out[from + k]);
            }
        }
    }
    return out;
}
}  // namespace png_detail
inline ImageRgb8 load_png(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open texture " + path);
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (d.size() < 8 || std::memcmp(d.data(), sig, 8) != 0) throw std::runtime_error(path + ": not a PNG (a git-LFS pointer stub?)");
    auto be32 = [&](size_t o) { return ((uint32_t)d[o] << 24) | ((uint32_t)d[o + 1] << 16) | ((uint32_t)d[o + 2] << 8) | d[o + 3]; };
    uint32_t w = 0, h = 0; int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat, plte;
    for (size_t o = 8; o + 12 <= d.size();) {
        uint32_t len = be32(o); std::string type((const char*)&d[o + 4], 4);
        if (o + 12 + len > d.size()) throw std::runtime_error(path + ": truncated chunk");
        const uint8_t* body = &d[o + 8];
        if (type == "IHDR") { w = be32(o + 8); h = be32(o + 12); depth = body[8]; ctype = body[9]; interlace = body[12]; }
        else if (type == "PLTE") plte.assign(body, body + len);
        else if (type == "IDAT") idat.insert(idat.end(), body, body + len);
        else if (type == "IEND") break;
        o += 12 + len;
    }
    if (!w || !h || interlace) throw std::runtime_error(path + ": unsupported PNG (interlaced or empty)");
    int ch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!ch || !(depth == 8 || depth == 16 || (ctype == 3 && depth <= 8) || (ctype == 0 && depth <= 8))) throw std::runtime_error(path + ": unsupported PNG colour type");
    std::vector<uint8_t> raw = png_detail::inflate(idat.data(), idat.size());
    size_t bpp = std::max<size_t>(1, (size_t)ch * depth / 8), stride = ((size_t)w * ch * depth + 7) / 8;
    if (raw.size() < (stride + 1) * h) throw std::runtime_error(path + ": image data too short");
    std::vector<uint8_t> cur(stride), prev(stride, 0);
    ImageRgb8 im; im.w = w; im.h = h; im.rgb.resize((size_t)w * h * 3);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t* line = &raw[(stride + 1) * y];
        int ft = line[0];
        for (size_t i = 0; i < stride; ++i) {
            int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0, x = line[1 + i];
            int v;
            switch (ft) {
                case 0: v = x; break; case 1: v = x + a; break; case 2: v = x + b; break; case 3: v = x + ((a + b) >> 1); break;
                case 4: { int pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c); v = x + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c)); break; }
                default: throw std::runtime_error(path + ": bad PNG filter");
            }
            cur[i] = (uint8_t)v;
        }
        for (uint32_t x = 0; x < w; ++x) {
            uint8_t* o = &im.rgb[((size_t)y * w + x) * 3];
            auto sample = [&](int k) -> uint8_t {           // k-th channel of pixel x as 8 bits (16-bit: high byte, like image's to_rgb8 up to rounding)
                if (depth == 16) return cur[((size_t)x * ch + k) * 2];
                if (depth == 8) return cur[(size_t)x * ch + k];
                size_t bit = (size_t)x * depth; int v = (cur[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
                return ctype == 3 ? (uint8_t)v : (uint8_t)(v * 255 / ((1 << depth) - 1));
            };
            if (ctype == 3) { size_t i = sample(0); if (3 * i + 2 >= plte.size()) throw std::runtime_error(path + ": palette index out of range"); o[0] = plte[3 * i]; o[1] = plte[3 * i + 1]; o[2] = plte[3 * i + 2]; }
            else if (ch <= 2) { o[0] = o[1] = o[2] = sample(0); }
            else { o[0] = sample(0); o[1] = sample(1); o[2] = sample(2); }
        }
        std::swap(cur, prev);
    }
    return im;
}
// float RGB environment maps: PFM ("PF", little or big endian, rows bottom-to-top) -> top-to-bottom h*w*3
inline std::vector<float> load_pfm(const std::string& path, uint32_t* w, uint32_t* h) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open environment map " + path);
    std::string magic; float scale;
    f >> magic >> *w >> *h >> scale; f.get();
    if (magic != "PF" || !*w || !*h) throw std::runtime_error(path + ": expected a colour PFM (PF)");
    std::vector<float> raw((size_t)*w * *h * 3);
    f.read((char*)raw.data(), (std::streamsize)(raw.size() * sizeof(float)));
    if (!f) throw std::runtime_error(path + ": truncated");
    if (scale > 0.0f) for (float& v : raw) { uint32_t u; std::memcpy(&u, &v, 4); u = __builtin_bswap32(u); std::memcpy(&v, &u, 4); }   // big endian
    std::vector<float> out(raw.size());
    for (uint32_t y = 0; y < *h; ++y) std::memcpy(&out[(size_t)y * *w * 3], &raw[(size_t)(*h - 1 - y) * *w * 3], (size_t)*w * 3 * sizeof(float));
    return out;
}
// the other way: top-to-bottom h*w*3 floats -> a little-endian colour PFM (scale -1), rows bottom to top; every value keeps its bits
// (the float output of the CLI's position and depth renderers)
inline void write_pfm(const std::string& path, const float* rgb, uint32_t w, uint32_t h) {
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "PF\n" << w << " " << h << "\n-1.0\n";
    for (uint32_t y = h; y-- > 0;) f.write((const char*)&rgb[(size_t)y * w * 3], (std::streamsize)((size_t)w * 3 * sizeof(float)));
    if (!f) throw std::runtime_error(path + ": write failed");
}
// float RGB environment maps as the reference reads them: OpenEXR through image::open(..).to_rgb32f() (environment_light.rs:30-41).
// Own reader for the scanline subset HDR skies ship in: single part, NO / ZIPS / ZIP compression (the zlib inflate above + OpenEXR's
// byte predictor and de-interleave), HALF or FLOAT channels R, G, B (other channels such as A are skipped), either line order.
// Returns top-to-bottom h*w*3.  PIZ / PXR24 / B44 / DWA, tiles, deep and multi-part files are refused with a message.
namespace exr_detail {
inline float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = s;
        else { int sh = 0; uint32_t mm = m; while (!(mm & 1024u)) { mm <<= 1; ++sh; } u = s | ((uint32_t)(113 - sh) << 23) | ((mm & 1023u) << 13); }   // subnormal
    } else if (e == 31) u = s | 0x7f800000u | (m << 13);
    else u = s | ((e + 112u) << 23) | (m << 13);
    float f; std::memcpy(&f, &u, 4); return f;
}
}
inline std::vector<float> load_exr(const std::string& path, uint32_t* w_out, uint32_t* h_out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open environment map " + path);
    std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t p = 0;
    auto need = [&](size_t n) { if (p + n > d.size()) throw std::runtime_error(path + ": truncated EXR"); };
    auto rd32 = [&]() { need(4); uint32_t v; std::memcpy(&v, &d[p], 4); p += 4; return v; };
    auto rdstr = [&]() { std::string s; for (;;) { need(1); char c = (char)d[p++]; if (!c) break; s.push_back(c); if (s.size() > 255) throw std::runtime_error(path + ": bad EXR string"); } return s; };
    if (rd32() != 20000630u) throw std::runtime_error(path + ": not an OpenEXR file");
    const uint32_t version = rd32();
    if ((version & 0xffu) != 2u || (version & 0x1a00u)) throw std::runtime_error(path + ": tiled / deep / multi-part EXR files are not supported (scanline only)");
    struct Chan { std::string name; uint32_t type; };
    std::vector<Chan> chans;
    int compression = -1, line_order = 0; int32_t win[4] = {0, 0, -1, -1}; bool have_win = false;
    for (;;) {
        std::string name = rdstr();
        if (name.empty()) break;
        std::string type = rdstr();
        const uint32_t size = rd32();
        need(size);
        const size_t q = p;
        const size_t q_end = q + size;                  // every read of this attribute stays below q_end (need(size) above: q_end <= d.size())
        auto attr_need = [&](size_t at, size_t n) { if (at > q_end || n > q_end - at) throw std::runtime_error(path + ": malformed EXR header attribute '" + name + "'"); };
        if (name == "channels") {
            size_t c = q;
            for (;;) {
                attr_need(c, 1);
                if (!d[c]) break;                                           // the list ends with an empty name
                Chan ch;
                for (;;) { attr_need(c, 1); const char k = (char)d[c++]; if (!k) break; ch.name.push_back(k); if (ch.name.size() > 255) throw std::runtime_error(path + ": bad EXR channel name"); }
                attr_need(c, 16);                                           // pixel type; pLinear + 3 reserved; xSampling; ySampling
                std::memcpy(&ch.type, &d[c], 4); c += 4 + 4;
                uint32_t xs, ys; std::memcpy(&xs, &d[c], 4); std::memcpy(&ys, &d[c + 4], 4); c += 8;
                if (xs != 1 || ys != 1) throw std::runtime_error(path + ": sub-sampled EXR channels are not supported");
                chans.push_back(ch);
                if (chans.size() > 1024) throw std::runtime_error(path + ": too many EXR channels");
            }
        } else if (name == "compression") { attr_need(q, 1); compression = d[q]; }
        else if (name == "dataWindow") { attr_need(q, 16); std::memcpy(win, &d[q], 16); have_win = true; }
        else if (name == "lineOrder") { attr_need(q, 1); line_order = d[q]; }
        p = q_end;
    }
    if (!have_win || chans.empty() || compression < 0) throw std::runtime_error(path + ": EXR header lacks channels / compression / dataWindow");
    if (compression != 0 && compression != 2 && compression != 3) throw std::runtime_error(path + ": EXR compression " + std::to_string(compression) + " is not supported (NONE, ZIPS, ZIP are)");
    // the window in 64-bit arithmetic: xMax < xMin, an overflowing extent or an absurd pixel count is a malformed file, not an allocation
    const int64_t w64 = (int64_t)win[2] - (int64_t)win[0] + 1, h64 = (int64_t)win[3] - (int64_t)win[1] + 1;
    if (w64 < 1 || h64 < 1 || w64 > 65536 || h64 > 65536 || w64 * h64 > ((int64_t)1 << 28)) throw std::runtime_error(path + ": EXR data window is empty or too large");
    const uint32_t w = (uint32_t)w64, h = (uint32_t)h64;
    int idx[3] = {-1, -1, -1};
    size_t line_bytes = 0; std::vector<size_t> chan_off(chans.size());
    for (size_t i = 0; i < chans.size(); ++i) {
        if (chans[i].type != 1 && chans[i].type != 2) throw std::runtime_error(path + ": EXR UINT channels are not supported");
        chan_off[i] = line_bytes; line_bytes += (size_t)w * (chans[i].type == 1 ? 2 : 4);
        if (chans[i].name == "R") idx[0] = (int)i;
        if (chans[i].name == "G") idx[1] = (int)i;
        if (chans[i].name == "B") idx[2] = (int)i;
    }
    if (idx[0] < 0 && chans.size() == 1) idx[0] = idx[1] = idx[2] = 0;      // a luminance-only file: grey (to_rgb32f does the same)
    if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0) throw std::runtime_error(path + ": EXR file has no R, G, B channels");
    const uint32_t lines_per_block = compression == 3 ? 16u : 1u, n_blocks = (h + lines_per_block - 1) / lines_per_block;
    need((size_t)n_blocks * 8); p += (size_t)n_blocks * 8;                    // the offset table: chunks are read in file order instead
    std::vector<float> out((size_t)w * h * 3);
    (void)line_order;                                                          // every chunk carries its own y
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const int32_t y0 = (int32_t)rd32(); const uint32_t size = rd32();
        need(size);
        if (y0 < win[1] || y0 > win[3]) throw std::runtime_error(path + ": EXR chunk outside the data window");
        const uint32_t rows = (uint32_t)std::min<int64_t>(lines_per_block, (int64_t)win[3] - (int64_t)y0 + 1);
        const size_t raw_size = line_bytes * rows;
        std::vector<uint8_t> raw;
        if (compression == 0 && size != raw_size) throw std::runtime_error(path + ": EXR chunk has the wrong size");
        if (compression == 0 || size == raw_size) raw.assign(d.begin() + (long)p, d.begin() + (long)(p + size));
        else {
            std::vector<uint8_t> t = png_detail::inflate(&d[p], size);
            if (t.size() != raw_size) throw std::runtime_error(path + ": EXR chunk inflates to the wrong size");
            for (size_t i = 1; i < t.size(); ++i) t[i] = (uint8_t)(t[i - 1] + t[i] - 128);          // predictor
            raw.resize(raw_size);
            const size_t half = (raw_size + 1) / 2;
            for (size_t i = 0; i < raw_size; ++i) raw[i] = (i & 1) ? t[half + i / 2] : t[i / 2];       // de-interleave the two halves
        }
        if (raw.size() != raw_size) throw std::runtime_error(path + ": EXR chunk has the wrong size");
        p += size;
        for (uint32_t r = 0; r < rows; ++r) {
            const uint8_t* line = &raw[line_bytes * r];
            float* o = &out[(size_t)(y0 - win[1] + (int32_t)r) * w * 3];
            for (int c = 0; c < 3; ++c) {
                const Chan& ch = chans[(size_t)idx[c]]; const uint8_t* src = line + chan_off[(size_t)idx[c]];
                for (uint32_t x = 0; x < w; ++x) {
                    if (ch.type == 1) { uint16_t hv; std::memcpy(&hv, src + 2 * x, 2); o[3 * x + c] = exr_detail::half_to_float(hv); }
                    else std::memcpy(&o[3 * x + c], src + 4 * x, 4);
                }
            }
        }
    }
    *w_out = w; *h_out = h;
    return out;
}
inline std::vector<float> load_float_image(const std::string& path, uint32_t* w, uint32_t* h) {   // by extension: .exr like the reference's sky, .pfm for the stand-in
    return path.size() >= 4 && path.compare(path.size() - 4, 4, ".exr") == 0 ? load_exr(path, w, h) : load_pfm(path, w, h);
}
inline ImageRgb8 load_image(const std::string& path) {      // by extension: .png like the reference's assets, .ppm for the synthetic stand-ins
    return path.size() >= 4 && path.compare(path.size() - 4, 4, ".png") == 0 ? load_png(path) : load_ppm(path);
}
struct RgbTexture { std::shared_ptr<ImageRgb8> img; static RgbTexture load_srgb(const std::string& p) { return {std::make_shared<ImageRgb8>(load_image(p))}; } };
struct NormalTexture { std::shared_ptr<ImageRgb8> img; bool flip_y; static NormalTexture load(const std::string& p, bool flip_y) { return {std::make_shared<ImageRgb8>(load_image(p)), flip_y}; } };
enum class SpectrumType { Albedo, Illuminant, Unbounded };      // texture/config.rs; Illuminant / Unbounded: emitter radiance (rgb_texture.rs:56-64)

// ------------------------------------------------------------------ parameters (scene/src/material/parameter.rs)
struct SpectrumParameter {
    bool is_texture = false; Spectrum spectrum; RgbTexture tex; SpectrumType tex_type = SpectrumType::Albedo;
    static SpectrumParameter constant(Spectrum s) { SpectrumParameter p; p.spectrum = std::move(s); return p; }
    static SpectrumParameter texture(RgbTexture t, SpectrumType ty) { SpectrumParameter p; p.is_texture = true; p.tex = std::move(t); p.tex_type = ty; return p; }
};
struct FloatTexture {                                          // texture/float_texture.rs:24-31 (gamma_corrected = false only)
    std::shared_ptr<ImageRgb8> img;
    static FloatTexture load(const std::string& p, bool gamma_corrected) {
        if (gamma_corrected) throw std::runtime_error("FloatTexture: gamma-corrected maps are not supported");
        return {std::make_shared<ImageRgb8>(load_image(p))};
    }
};
struct FloatParameter {                                        // material/parameter.rs:58-83
    float v = 0.0f; std::shared_ptr<ImageRgb8> tex;
    static FloatParameter constant(float x) { FloatParameter p; p.v = x; return p; }
    static FloatParameter texture(FloatTexture t) { FloatParameter p; p.tex = std::move(t.img); return p; }
};
struct NormalParameter {
    bool has = false; NormalTexture tex{};
    static NormalParameter none() { return {}; }
    static NormalParameter texture(NormalTexture t) { NormalParameter p; p.has = true; p.tex = std::move(t); return p; }
};

// ------------------------------------------------------------------ materials (scene/src/material/impls/*.rs)
struct Material {
    uint32_t type = 0; SpectrumParameter color; NormalParameter normal; float intensity = 1; Spectrum eta; bool thin = false; float roughness = 0;
    float metallic = 0, ior = 1.5f, clearcoat_ior = 1.5f, clearcoat_roughness = 0, clearcoat_thickness = 0; SpectrumParameter clearcoat_tint;
    Spectrum k;   // metal: extinction coefficient
    std::shared_ptr<ImageRgb8> metallic_tex, roughness_tex, clearcoat_thickness_tex;   // FloatParameter::texture (grey image replicated to RGB)
    std::shared_ptr<ImageRgb8> intensity_tex;                                          // emissive: FloatParameter::texture intensity
};
struct LambertMaterial { static Material create(SpectrumParameter albedo, NormalParameter n) { Material m; m.type = MI355PT_MAT_LAMBERT; m.color = std::move(albedo); m.normal = std::move(n); return m; } };
struct EmissiveMaterial { static Material create(SpectrumParameter radiance, FloatParameter intensity) { Material m; m.type = MI355PT_MAT_EMISSIVE; m.color = std::move(radiance); m.intensity = intensity.v; m.intensity_tex = intensity.tex; return m; } };
enum class GlassType { Bk7, Sf11 };
struct GlassMaterial {
    static Material create(GlassType t, NormalParameter n, bool thin, FloatParameter rough) {
        Material m; m.type = MI355PT_MAT_GLASS; m.eta = t == GlassType::Sf11 ? presets::glass_sf11_eta() : presets::glass_bk7_eta();
        m.color = SpectrumParameter::constant(ConstantSpectrum::create(1.0f)); m.normal = std::move(n); m.thin = thin; m.roughness = rough.v; m.roughness_tex = rough.tex; return m;
    }
};
struct PlasticMaterial {
    static Material create(float eta, SpectrumParameter color, NormalParameter n, bool thin, FloatParameter rough) {
        Material m; m.type = MI355PT_MAT_PLASTIC; m.eta = ConstantSpectrum::create(eta); m.color = std::move(color); m.normal = std::move(n); m.thin = thin; m.roughness = rough.v; m.roughness_tex = rough.tex; return m;
    }
};
enum class MetalType { Gold, Silver, Copper, Aluminum, Brass };                       // metal_material.rs:16-29
struct MetalMaterial {                                                                 // metal_material.rs:44-92
    static Material create(MetalType t, NormalParameter n, FloatParameter rough) {
        Material m; m.type = MI355PT_MAT_METAL; m.normal = std::move(n); m.roughness = rough.v; m.roughness_tex = rough.tex;
        m.color = SpectrumParameter::constant(ConstantSpectrum::create(1.0f));
        switch (t) {
            case MetalType::Gold: m.eta = presets::au_eta(); m.k = presets::au_k(); break;
            case MetalType::Silver: m.eta = presets::ag_eta(); m.k = presets::ag_k(); break;
            case MetalType::Copper: m.eta = presets::cu_eta(); m.k = presets::cu_k(); break;
            case MetalType::Aluminum: m.eta = presets::al_eta(); m.k = presets::al_k(); break;
            case MetalType::Brass: m.eta = presets::cu_zn_eta(); m.k = presets::cu_zn_k(); break;
        }
        return m;
    }
};
struct SimplePbrMaterial {                                                             // simple_pbr_material.rs:29-45
    static Material create(SpectrumParameter base_color, FloatParameter metallic, FloatParameter roughness, NormalParameter n, FloatParameter ior) {
        Material m; m.type = MI355PT_MAT_SIMPLE_PBR; m.color = std::move(base_color); m.metallic = metallic.v; m.roughness = roughness.v;
        m.metallic_tex = metallic.tex; m.roughness_tex = roughness.tex;
        m.normal = std::move(n); m.ior = ior.v; return m;
    }
};
struct SimpleClearcoatPbrMaterial {
    static Material create(SpectrumParameter base_color, FloatParameter metallic, FloatParameter roughness, NormalParameter n, FloatParameter ior,
                           FloatParameter cc_ior, FloatParameter cc_rough, SpectrumParameter cc_tint, FloatParameter cc_thickness) {
        Material m; m.type = MI355PT_MAT_CLEARCOAT; m.color = std::move(base_color); m.metallic = metallic.v; m.roughness = roughness.v; m.normal = std::move(n);
        m.metallic_tex = metallic.tex; m.roughness_tex = roughness.tex;
        m.ior = ior.v; m.clearcoat_ior = cc_ior.v; m.clearcoat_roughness = cc_rough.v; m.clearcoat_tint = std::move(cc_tint); m.clearcoat_thickness = cc_thickness.v;
        m.clearcoat_thickness_tex = cc_thickness.tex; return m;
    }
};

// ------------------------------------------------------------------ Transform (math/src/transform.rs:76-162), column-major glam::Mat4
struct Transform {
    float m[16];
    static Transform identity() { Transform t{}; for (int i = 0; i < 16; ++i) t.m[i] = (i % 5 == 0) ? 1.0f : 0.0f; return t; }
    static Transform mul(const Transform& a, const Transform& b) {
        Transform o{};
        for (int c = 0; c < 4; ++c) for (int r = 0; r < 4; ++r) {
            float s = a.m[r] * b.m[4 * c]; s = s + a.m[4 + r] * b.m[4 * c + 1]; s = s + a.m[8 + r] * b.m[4 * c + 2]; s = s + a.m[12 + r] * b.m[4 * c + 3];
            o.m[4 * c + r] = s;
        }
        return o;
    }
    Transform rotate_y(float angle_rad) const {      // .rotate(Quat::from_euler(XYZ, 0, a, 0)) — left-multiplies (:134-137)
        // glam: q = (0, sin(a/2), 0, cos(a/2)); Mat4::from_quat builds 1 - y*(y+y) and w*(y+y)
        float y = std::sin(angle_rad * 0.5f), w = std::cos(angle_rad * 0.5f);
        float y2 = y + y, yy = y * y2, wy = w * y2;
        Transform r = identity();
        r.m[0] = 1.0f - yy; r.m[2] = -wy; r.m[8] = wy; r.m[10] = 1.0f - yy;
        return mul(r, *this);
    }
    static Transform from_scale(Vec3 v) { Transform s = identity(); s.m[0] = v.x; s.m[5] = v.y; s.m[10] = v.z; return s; }   // :119-122
    Transform scale(Vec3 v) const { Transform s = identity(); s.m[0] = v.x; s.m[5] = v.y; s.m[10] = v.z; return mul(s, *this); }
    static Transform from_translate(Vec3 v) { return identity().translate(v); }                 // :94-97
    static Transform from_rotate_y(float angle_rad) { return identity().rotate_y(angle_rad); }   // from_rotate(Quat::from_rotation_y(a)) :112-115
    Transform translate(Vec3 v) const { Transform t = identity(); t.m[12] = v.x; t.m[13] = v.y; t.m[14] = v.z; return mul(t, *this); }
};

// ------------------------------------------------------------------ Camera (renderer/src/camera.rs:14-92)
class Camera {
public:
    Camera(float fov, uint32_t width, uint32_t height) { c_.fov_deg = fov; c_.width = width; c_.height = height; set_look_to({0, 0, 0}, {0, 0, -1}, {0, 1, 0}); }
    void set_look_to(Vec3 p, Vec3 d, Vec3 u) {
        c_.position[0] = p.x; c_.position[1] = p.y; c_.position[2] = p.z; c_.direction[0] = d.x; c_.direction[1] = d.y; c_.direction[2] = d.z;
        c_.up[0] = u.x; c_.up[1] = u.y; c_.up[2] = u.z;
    }
    const mi355pt_camera& raw() const { return c_; }
private:
    mi355pt_camera c_{};
};

// ------------------------------------------------------------------ OBJ loading (geometry/impls/triangle_mesh.rs:141-242)
struct TriangleMeshData { std::vector<float> pos, nrm, uv, tangent; std::vector<uint32_t> idx; };
inline Vec3 v_sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline Vec3 v_cross(Vec3 a, Vec3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline float v_dot(Vec3 a, Vec3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
inline Vec3 v_norm(Vec3 a) { float r = 1.0f / std::sqrt(v_dot(a, a)); return {a.x * r, a.y * r, a.z * r}; }
inline bool v_nan(Vec3 a) { return std::isnan(a.x) || std::isnan(a.y) || std::isnan(a.z); }

// per-triangle tangents with the reference's fallback rules (geometry/impls/triangle_mesh.rs:181-226)
inline void compute_tangents(TriangleMeshData& out) {
    if (out.uv.empty()) return;
    {
        auto P = [&](uint32_t i) { return Vec3{out.pos[3 * i], out.pos[3 * i + 1], out.pos[3 * i + 2]}; };
        auto fallback = [](Vec3 e1, Vec3 e2) {
            Vec3 c = v_cross(e1, e2);
            if (v_dot(c, c) < 1e-12f) return Vec3{1, 0, 0};
            Vec3 n = v_norm(v_norm(c));
            Vec3 cand = std::fabs(n.x) > 0.999f ? Vec3{0, 1, 0} : Vec3{1, 0, 0};
            float pm = v_dot(n, cand);
            return v_norm(Vec3{cand.x - n.x * pm, cand.y - n.y * pm, cand.z - n.z * pm});
        };
        for (size_t t = 0; t < out.idx.size() / 3; ++t) {
            uint32_t i0 = out.idx[3 * t], i1 = out.idx[3 * t + 1], i2 = out.idx[3 * t + 2];
            Vec3 e1 = v_sub(P(i1), P(i0)), e2 = v_sub(P(i2), P(i0));
            float du1 = out.uv[2 * i1] - out.uv[2 * i0], dv1 = out.uv[2 * i1 + 1] - out.uv[2 * i0 + 1];
            float du2 = out.uv[2 * i2] - out.uv[2 * i0], dv2 = out.uv[2 * i2 + 1] - out.uv[2 * i0 + 1];
            float den = du1 * dv2 - dv1 * du2;
            float r = 1.0f / den;
            Vec3 tg{r * (e1.x * dv2 - e2.x * dv1), r * (e1.y * dv2 - e2.y * dv1), r * (e1.z * dv2 - e2.z * dv1)};
            if (std::fabs(den) < 1e-6f) tg = fallback(e1, e2);
            else { tg = v_norm(tg); if (v_nan(tg)) tg = fallback(e1, e2); }
            out.tangent.insert(out.tangent.end(), {tg.x, tg.y, tg.z});
        }
    }
}

// Area-weighted vertex normals of a mesh whose positions changed (--mesh-wave, main.cpp): every triangle adds its un-normalised cross
// product — twice its area along its normal — to its three vertices; the library normalises what it is given (mi355pt_scene_deform_meshes).
// A vertex no triangle with area touches keeps the normal it had.
inline std::vector<float> area_weighted_normals(const TriangleMeshData& m, const std::vector<float>& pos) {
    std::vector<double> acc(pos.size(), 0.0);
    auto P = [&](uint32_t i) { return Vec3{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}; };
    for (size_t t = 0; t + 2 < m.idx.size(); t += 3) {
        const Vec3 n = v_cross(v_sub(P(m.idx[t + 1]), P(m.idx[t])), v_sub(P(m.idx[t + 2]), P(m.idx[t])));
        for (int k = 0; k < 3; ++k) { acc[3 * m.idx[t + k]] += n.x; acc[3 * m.idx[t + k] + 1] += n.y; acc[3 * m.idx[t + k] + 2] += n.z; }
    }
    std::vector<float> nrm(m.nrm);
    for (size_t v = 0; v * 3 < pos.size(); ++v) {
        const double l = std::sqrt(acc[3 * v] * acc[3 * v] + acc[3 * v + 1] * acc[3 * v + 1] + acc[3 * v + 2] * acc[3 * v + 2]);
        if (l > 0.0) for (int a = 0; a < 3; ++a) nrm[3 * v + a] = (float)(acc[3 * v + a] / l);
    }
    return nrm;
}

inline TriangleMeshData load_obj_file(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open OBJ " + path);
    std::vector<Vec3> v, vn; std::vector<std::array<float, 2>> vt;
    std::map<std::tuple<int, int, int>, uint32_t> remap;      // tobj single_index: one vertex per distinct (v, vt, vn)
    TriangleMeshData out;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ls(line);
        std::string tag; ls >> tag;
        if (tag == "v") { Vec3 p; ls >> p.x >> p.y >> p.z; v.push_back(p); }
        else if (tag == "vn") { Vec3 p; ls >> p.x >> p.y >> p.z; vn.push_back(p); }
        else if (tag == "vt") { std::array<float, 2> t; ls >> t[0] >> t[1]; vt.push_back(t); }
        else if (tag == "f") {
            std::vector<uint32_t> face;
            std::string tok;
            while (ls >> tok) {
                int a = 0, b = 0, c = 0;
                if (std::sscanf(tok.c_str(), "%d/%d/%d", &a, &b, &c) == 3) {}
                else if (std::sscanf(tok.c_str(), "%d//%d", &a, &c) == 2) { b = 0; }
                else if (std::sscanf(tok.c_str(), "%d/%d", &a, &b) == 2) { c = 0; }
                else { std::sscanf(tok.c_str(), "%d", &a); }
                auto key = std::make_tuple(a, b, c);
                auto it = remap.find(key);
                if (it == remap.end()) {
                    uint32_t id = (uint32_t)(out.pos.size() / 3);
                    Vec3 p = v.at((size_t)a - 1);
                    out.pos.insert(out.pos.end(), {p.x, p.y, p.z});
                    if (c > 0) { Vec3 n = vn.at((size_t)c - 1); out.nrm.insert(out.nrm.end(), {n.x, n.y, n.z}); }
                    if (b > 0) { auto t = vt.at((size_t)b - 1); out.uv.insert(out.uv.end(), {t[0], t[1]}); }
                    it = remap.emplace(key, id).first;
                }
                face.push_back(it->second);
            }
            for (size_t k = 1; k + 1 < face.size(); ++k) { out.idx.push_back(face[0]); out.idx.push_back(face[k]); out.idx.push_back(face[k + 1]); }   // triangulate
        }
    }
    if (out.nrm.size() != out.pos.size()) throw std::runtime_error(path + ": every vertex needs a normal");
    if (!out.uv.empty() && out.uv.size() / 2 != out.pos.size() / 3) throw std::runtime_error(path + ": inconsistent texcoords");
    compute_tangents(out);
    return out;
}

// ------------------------------------------------------------------ Scene
struct GeometryIndex { uint32_t id; };
struct GeometryPrimitive { GeometryIndex geometry_index; Material surface_material; Transform transform; };   // CreatePrimitiveDesc::GeometryPrimitive
// CreatePrimitiveDesc::{SingleTriangle,PointLight,SpotLight,DirectionalLight}Primitive (primitive/create_desc.rs:17-66)
struct SingleTrianglePrimitive { Vec3 positions[3]; Vec3 normals[3]; float uvs[3][2]; Material surface_material; Transform transform; };
struct PointLightPrimitive { float intensity; Spectrum spectrum; Transform transform; };
struct EnvironmentLightPrimitive { float intensity; std::string texture_path; Transform transform; };   // .exr like the reference, or .pfm
struct SpotLightPrimitive { float angle_inner, angle_outer, intensity; Spectrum spectrum; Transform transform; };
struct DirectionalLightPrimitive { float intensity; Spectrum spectrum; Transform transform; };

class Scene {
public:
    Scene() {
        check(mi355pt_scene_create(&s_), "mi355pt_scene_create");
        std::ifstream t(data_dir() + "/srgb_table.bin", std::ios::binary);
        if (!t) throw std::runtime_error("srgb_table.bin not found under " + data_dir() + " (run __graft_entry__.build())");
        std::vector<float> tab(64 + 3 * 64 * 64 * 64 * 3);
        t.read((char*)tab.data(), (std::streamsize)(tab.size() * sizeof(float)));
        check(mi355pt_scene_set_rgb2spec(s_, tab.data(), tab.size()), "mi355pt_scene_set_rgb2spec");
    }
    ~Scene() { mi355pt_scene_destroy(s_); }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;

    GeometryIndex load_obj(const std::string& path) {
        TriangleMeshData m = load_obj_file(path);
        uint32_t id;
        check(mi355pt_scene_add_mesh(s_, m.pos.data(), m.nrm.data(), m.uv.empty() ? nullptr : m.uv.data(), m.tangent.empty() ? nullptr : m.tangent.data(),
                                     m.idx.data(), (uint32_t)(m.pos.size() / 3), (uint32_t)(m.idx.size() / 3), &id), "mi355pt_scene_add_mesh");
        meshes_.push_back(std::move(m));
        return {id};
    }
    void create_primitive(const GeometryPrimitive& d) {
        mi355pt_material_desc md{};
        const Material& m = d.surface_material;
        md.type = m.type; md.color = lower(m.color); md.normal_tex = MI355PT_NONE; md.metallic_tex = md.roughness_tex = MI355PT_NONE;
        if (m.metallic_tex) md.metallic_tex = add_tex(*m.metallic_tex);
        if (m.roughness_tex) md.roughness_tex = add_tex(*m.roughness_tex);
        md.clearcoat_thickness_tex = m.clearcoat_thickness_tex ? add_tex(*m.clearcoat_thickness_tex) : MI355PT_NONE;
        md.intensity_tex = (m.type == MI355PT_MAT_EMISSIVE && m.intensity_tex) ? add_tex(*m.intensity_tex) : MI355PT_NONE;
        if (m.normal.has) { md.normal_tex = add_tex(*m.normal.tex.img); md.normal_flip_y = m.normal.tex.flip_y ? 1 : 0; }
        md.intensity = m.intensity; md.thin = m.thin ? 1 : 0; md.roughness = m.roughness;
        if (m.type == MI355PT_MAT_GLASS || m.type == MI355PT_MAT_PLASTIC || m.type == MI355PT_MAT_METAL) md.eta = lower_spectrum(m.eta);
        if (m.type == MI355PT_MAT_METAL) md.k = lower_spectrum(m.k);
        md.metallic = m.metallic; md.ior = m.ior; md.clearcoat_ior = m.clearcoat_ior; md.clearcoat_roughness = m.clearcoat_roughness;
        md.clearcoat_thickness = m.clearcoat_thickness;
        if (m.type == MI355PT_MAT_CLEARCOAT) md.clearcoat_tint = lower(m.clearcoat_tint);
        uint32_t mat;
        check(mi355pt_scene_add_material(s_, &md, &mat), "mi355pt_scene_add_material");
        if (material_descs_.size() <= mat) { material_descs_.resize(mat + 1); has_material_.resize(mat + 1, 0); }
        material_descs_[mat] = md; has_material_[mat] = 1;
        check(mi355pt_scene_add_instance(s_, d.geometry_index.id, mat, d.transform.m), "mi355pt_scene_add_instance");
        instance_l2w_.emplace_back(d.transform.m, d.transform.m + 16);
    }
    void create_primitive(const SingleTrianglePrimitive& d) {      // lowered to a one-triangle mesh with load_obj's tangent rule
        TriangleMeshData m;
        for (int i = 0; i < 3; ++i) {
            m.pos.insert(m.pos.end(), {d.positions[i].x, d.positions[i].y, d.positions[i].z});
            m.nrm.insert(m.nrm.end(), {d.normals[i].x, d.normals[i].y, d.normals[i].z});
            m.uv.insert(m.uv.end(), {d.uvs[i][0], d.uvs[i][1]});
        }
        m.idx = {0, 1, 2};
        compute_tangents(m);
        uint32_t id;
        check(mi355pt_scene_add_mesh(s_, m.pos.data(), m.nrm.data(), m.uv.data(), m.tangent.data(), m.idx.data(), 3, 1, &id), "mi355pt_scene_add_mesh");
        meshes_.push_back(std::move(m));
        create_primitive(GeometryPrimitive{{id}, d.surface_material, d.transform});
    }
    void create_primitive(const EnvironmentLightPrimitive& d) {
        uint32_t w = 0, h = 0;
        std::vector<float> rgb = load_float_image(d.texture_path, &w, &h);                 // EXR (environment_light.rs:30-41) or PFM
        mi355pt_spectrum d65 = lower_spectrum(presets::cie_illum_d6500());       // rgb_illuminant_spectrum.rs:28
        check(mi355pt_scene_add_environment_light(s_, d.intensity, rgb.data(), w, h, d.transform.m, d65.id), "mi355pt_scene_add_environment_light");
        EnvDesc e; e.intensity = d.intensity; std::memcpy(e.l2w, d.transform.m, sizeof(e.l2w));
        envs_.push_back(e);
    }
    void create_primitive(const PointLightPrimitive& d) { add_light(MI355PT_LIGHT_POINT, d.intensity, 0, 0, d.spectrum, d.transform); }
    void create_primitive(const SpotLightPrimitive& d) { add_light(MI355PT_LIGHT_SPOT, d.intensity, d.angle_inner, d.angle_outer, d.spectrum, d.transform); }
    void create_primitive(const DirectionalLightPrimitive& d) { add_light(MI355PT_LIGHT_DIRECTIONAL, d.intensity, 0, 0, d.spectrum, d.transform); }
    // (LUTs are uploaded by mi355pt_scene_build: presets::cie_illum_d6500(), which AlbedoRenderer multiplies with — albedo_renderer.rs:60 —,
    // is lowered before it; every scene carries that one 470-float LUT whichever renderer runs)
    void build(const Camera& cam) {
        d65_lut_ = lower_spectrum(presets::cie_illum_d6500()).id;
        check(mi355pt_scene_build(s_, &cam.raw()), "mi355pt_scene_build");
    }
    // EXTENSION (include/mi355pt_rebase.h): the built scene follows a camera TRANSLATION on the device — vertices re-based, both trees
    // refit — instead of being built again; falls back to the full build where that would not give a fresh lowering's records
    mi355pt_move_result move_camera(const Camera& cam) {
        mi355pt_move_result r{};
        check(mi355pt_scene_move_camera(s_, &cam.raw(), &r), "mi355pt_scene_move_camera");
        return r;
    }
    // EXTENSION (include/mi355pt_instances.h): instances of the built scene take new local_to_world matrices (column-major, 16 floats each,
    // ids strictly ascending) on the device — positions, shading normals, light tables, both trees refit, the tree's SAH cost reported —;
    // an instance that will move is marked before build().  Across a move the temporal accumulation takes the object motion vectors of
    // include/mi355pt_motion.h: ids_device() says which instance a pixel shows, motion_table() where each instance's points were a frame ago
    void ids_device(const mi355pt_camera& cam, const mi355pt_params& p, uint32_t* d_ids) const {
        check(mi355pt_render_ids_device(s_, &cam, &p, d_ids, nullptr, nullptr), "mi355pt_render_ids_device");
    }
    // every instance's local_to_world in the previous frame (n x 16, column-major) against the scene's current ones -> instance_count() + 1 records
    std::vector<mi355pt_motion_xform> motion_table(const mi355pt_camera& cur, const mi355pt_camera& prev, const std::vector<float>& l2w_prev) const {
        std::vector<float> l2w_cur;
        for (const std::vector<float>& m : instance_l2w_) l2w_cur.insert(l2w_cur.end(), m.begin(), m.end());
        std::vector<mi355pt_motion_xform> out(instance_l2w_.size() + 1);
        check(mi355pt_motion_table(&cur, &prev, l2w_cur.data(), l2w_prev.data(), (uint32_t)instance_l2w_.size(), out.data()), "mi355pt_motion_table");
        return out;
    }
    // include/mi355pt_flow.h: flow_mark() keeps the current triangle positions as last frame's, flow_device() gives every pixel its motion record
    // (and its id) against the mark, flow_marked() says whether the mark survived the moves since (a build drops it)
    void flow_mark() { check(mi355pt_scene_flow_mark(s_, nullptr), "mi355pt_scene_flow_mark"); }
    bool flow_marked() const { return mi355pt_scene_flow_marked(s_) != 0; }
    void flow_device(const mi355pt_camera& cam, const mi355pt_params& p, mi355pt_flow_pixel* d_flow, uint32_t* d_ids) const {
        check(mi355pt_render_flow_device(s_, &cam, &p, d_flow, d_ids, nullptr, nullptr), "mi355pt_render_flow_device");
    }
    void set_instance_dynamic(uint32_t instance) { check(mi355pt_scene_set_instance_dynamic(s_, instance, 1), "mi355pt_scene_set_instance_dynamic"); }
    mi355pt_instance_move_result move_instances(const Camera& cam, const std::vector<uint32_t>& ids, const std::vector<float>& matrices, float rebuild_above = 0.0f) {
        mi355pt_instance_move_params p{rebuild_above};
        mi355pt_instance_move_result r{};
        check(mi355pt_scene_move_instances(s_, &cam.raw(), ids.data(), matrices.data(), (uint32_t)ids.size(), &p, &r), "mi355pt_scene_move_instances");
        for (size_t k = 0; k < ids.size(); ++k) instance_l2w_[ids[k]].assign(matrices.begin() + 16 * (long)k, matrices.begin() + 16 * (long)(k + 1));
        return r;
    }
    // EXTENSION (include/mi355pt_deform.h): meshes of the built scene take new positions and normals (tangents stay) on the device — the
    // local records replaced, then the instance move's sequence —; geoms strictly ascending, the arrays sized like the mesh's own
    mi355pt_instance_move_result deform_meshes(const Camera& cam, const std::vector<uint32_t>& geoms, const std::vector<std::vector<float>>& pos,
                                               const std::vector<std::vector<float>>& nrm, float rebuild_above = 0.0f) {
        std::vector<mi355pt_mesh_update> ups(geoms.size());
        for (size_t k = 0; k < geoms.size(); ++k) ups[k] = mi355pt_mesh_update{geoms[k], pos[k].data(), nrm[k].data(), nullptr};
        mi355pt_instance_move_params p{rebuild_above};
        mi355pt_instance_move_result r{};
        check(mi355pt_scene_deform_meshes(s_, &cam.raw(), ups.data(), (uint32_t)ups.size(), &p, &r), "mi355pt_scene_deform_meshes");
        for (size_t k = 0; k < geoms.size(); ++k) { meshes_[geoms[k]].pos = pos[k]; meshes_[geoms[k]].nrm = nrm[k]; }
        return r;
    }
    // EXTENSION (include/mi355pt_edit.h): materials, delta lights and environment lights of the built scene take new descriptions in place —
    // the small records lowered again and uploaded, one launch when a material changed its class —; ids strictly ascending in each list.
    // The mirror keeps what the scene was described with / last edited to: material_desc(), light_desc(), env_intensity(), env_transform()
    mi355pt_edit_result edit(const Camera& cam, const std::vector<mi355pt_material_edit>& materials, const std::vector<mi355pt_light_edit>& lights,
                             const std::vector<mi355pt_env_edit>& envs) {
        const mi355pt_scene_edits e{materials.data(), (uint32_t)materials.size(), lights.data(), (uint32_t)lights.size(), envs.data(), (uint32_t)envs.size()};
        mi355pt_edit_result r{};
        check(mi355pt_scene_edit(s_, &cam.raw(), &e, &r), "mi355pt_scene_edit");
        for (const mi355pt_material_edit& m : materials) material_descs_[m.mat] = m.desc;
        for (const mi355pt_light_edit& l : lights) light_descs_[l.light] = l.desc;
        for (const mi355pt_env_edit& v : envs) { envs_[v.env].intensity = v.intensity; if (v.local_to_world) std::memcpy(envs_[v.env].l2w, v.local_to_world, sizeof(envs_[v.env].l2w)); }
        return r;
    }
    uint32_t material_count() const { return (uint32_t)material_descs_.size(); }
    bool has_material(uint32_t mat) const { return mat < has_material_.size() && has_material_[mat] != 0; }      // (false: a light's hidden material)
    const mi355pt_material_desc& material_desc(uint32_t mat) const { return material_descs_[mat]; }
    uint32_t light_count() const { return (uint32_t)light_descs_.size(); }                                       // delta lights, in creation order
    const mi355pt_light_desc& light_desc(uint32_t light) const { return light_descs_[light]; }
    uint32_t env_count() const { return (uint32_t)envs_.size(); }
    float env_intensity(uint32_t env) const { return envs_[env].intensity; }
    const float* env_transform(uint32_t env) const { return envs_[env].l2w; }
    uint32_t mesh_count() const { return (uint32_t)meshes_.size(); }
    const TriangleMeshData& mesh(uint32_t geom) const { return meshes_[geom]; }      // as loaded / last deformed
    uint32_t instance_count() const { return (uint32_t)instance_l2w_.size(); }
    const float* instance_transform(uint32_t instance) const { return instance_l2w_[instance].data(); }   // local_to_world as described / last moved
    // Scene::build over the first `n_devices` GPUs of the node (mi355pt_scene_build_multi): RendererImage::render then shards the frame
    void build_multi(const Camera& cam, int n_devices) {
        std::vector<int> ids((size_t)n_devices);
        for (int i = 0; i < n_devices; ++i) ids[(size_t)i] = i;
        check(mi355pt_scene_build_multi(s_, &cam.raw(), n_devices, ids.data()), "mi355pt_scene_build_multi");
        multi_ = true;
    }
    bool multi() const { return multi_; }
    uint32_t d65_lut() const { return d65_lut_; }      // LUT470 id of presets::cie_illum_d6500() (MI355PT_NONE before build())
    const mi355pt_scene* raw() const { return s_; }

private:
    std::vector<std::vector<float>> instance_l2w_;      // by instance id
    std::vector<TriangleMeshData> meshes_;              // by geometry id
    struct EnvDesc { float intensity = 1.0f; float l2w[16]; };
    std::vector<mi355pt_material_desc> material_descs_; // by material id (the lights' hidden materials leave gaps: has_material_)
    std::vector<uint8_t> has_material_;
    std::vector<mi355pt_light_desc> light_descs_;       // by delta-light id
    std::vector<EnvDesc> envs_;                         // by environment-light id
    void add_light(uint32_t kind, float intensity, float a_in, float a_out, const Spectrum& sp, const Transform& t) {
        mi355pt_light_desc ld{}; ld.kind = kind; ld.intensity = intensity; ld.angle_inner = a_in; ld.angle_outer = a_out;
        ld.spectrum = lower_spectrum(sp); std::memcpy(ld.local_to_world, t.m, sizeof(ld.local_to_world));
        check(mi355pt_scene_add_delta_light(s_, &ld), "mi355pt_scene_add_delta_light");
        light_descs_.push_back(ld);
    }
    uint32_t add_tex(const ImageRgb8& im) { uint32_t id; check(mi355pt_scene_add_tex_rgb8(s_, im.rgb.data(), im.w, im.h, &id), "mi355pt_scene_add_tex_rgb8"); return id; }
    mi355pt_spectrum lower_spectrum(const Spectrum& sp) {
        mi355pt_spectrum s = sp.s;
        if (s.kind == MI355PT_SPEC_LUT470) check(mi355pt_scene_add_lut470(s_, sp.lut.data(), &s.id), "mi355pt_scene_add_lut470");
        return s;
    }
    mi355pt_spectrum lower(const SpectrumParameter& p) {
        if (!p.is_texture) return lower_spectrum(p.spectrum);
        mi355pt_spectrum s{}; s.id = add_tex(*p.tex.img);
        s.kind = p.tex_type == SpectrumType::Albedo ? MI355PT_SPEC_TEXTURE_ALBEDO_SRGB : (p.tex_type == SpectrumType::Illuminant ? MI355PT_SPEC_TEXTURE_ILLUMINANT_SRGB : MI355PT_SPEC_TEXTURE_UNBOUNDED_SRGB);
        if (p.tex_type == SpectrumType::Illuminant) s.c[0] = (float)lower_spectrum(presets::cie_illum_d6500()).id;     // RgbIlluminantSpectrum's illuminant (rgb_illuminant_spectrum.rs:27)
        return s;
    }
    mi355pt_scene* s_ = nullptr;
    bool multi_ = false;
    uint32_t d65_lut_ = MI355PT_NONE;
};

// ------------------------------------------------------------------ renderers (renderer/src/renderer.rs:84-149, main.rs:142-237)
enum class SamplerKind { Random = MI355PT_SAMPLER_RANDOM, ZSobol = MI355PT_SAMPLER_SOBOL };
struct RendererArgs { uint32_t width, height, spp, seed; const Scene* scene; const Camera* camera; };
// (aov: -1 = a path renderer; MI355PT_AOV_* = NormalRenderer / AlbedoRenderer / the shading-normal extension, which take only the args)
struct SrgbRenderer { RendererArgs args; uint32_t strategy; float exposure; uint32_t max_depth; int aov = -1; };
inline SrgbRenderer SrgbRendererPt(RendererArgs a, float exposure, uint32_t max_depth) { return {a, MI355PT_STRATEGY_PT, exposure, max_depth}; }
inline SrgbRenderer SrgbRendererNee(RendererArgs a, float exposure, uint32_t max_depth) { return {a, MI355PT_STRATEGY_NEE, exposure, max_depth}; }
inline SrgbRenderer SrgbRendererMis(RendererArgs a, float exposure, uint32_t max_depth) { return {a, MI355PT_STRATEGY_MIS, exposure, max_depth}; }
// NormalRenderer::new(args) / AlbedoRenderer::new(args) (renderer/normal_renderer.rs:17-21, albedo_renderer.rs:21-25; main.rs:155-186)
inline SrgbRenderer NormalRenderer(RendererArgs a) { return {a, MI355PT_STRATEGY_PT, 1.0f, 0u, MI355PT_AOV_NORMAL}; }
inline SrgbRenderer AlbedoRenderer(RendererArgs a) { return {a, MI355PT_STRATEGY_PT, 1.0f, 0u, MI355PT_AOV_ALBEDO}; }
// extension, no reference counterpart: the render-space shading normal of every surface (MI355PT_AOV_SHADING_NORMAL)
inline SrgbRenderer ShadingNormalRenderer(RendererArgs a) { return {a, MI355PT_STRATEGY_PT, 1.0f, 0u, MI355PT_AOV_SHADING_NORMAL}; }

class RendererImage {
public:
    RendererImage(uint32_t w, uint32_t h, SrgbRenderer r) : pixels_((size_t)w * h * 3, 0.0f), w_(w), h_(h), r_(r) {}
    // RendererImage::render::<S>() — the seam: one call into the HIP library fills `pixels`
    // (albedo_lut: mi355pt_params.albedo_lut, an option outside the reference's CLI; 0 = the reference's estimator)
    mi355pt_params params(SamplerKind sampler, bool albedo_lut = false) const {
        mi355pt_params p{};
        p.spp = r_.args.spp; p.seed = r_.args.seed; p.max_depth = r_.max_depth; p.strategy = r_.strategy; p.sampler = (uint32_t)sampler;
        p.exposure = r_.exposure; p.shard_index = 0; p.shard_count = 1; p.albedo_lut = albedo_lut ? 1u : 0u;
        return p;
    }
    double render(SamplerKind sampler, bool albedo_lut = false) {
        const mi355pt_params p = params(sampler, albedo_lut);
        if (r_.aov >= 0) {                                  // RendererImage::<NormalRenderer | AlbedoRenderer>::render (main.rs:155-186)
            if (r_.args.scene->multi()) throw std::runtime_error("the AOV renderers run on one GPU (mi355pt_render_multi has no AOV form)");
            mi355pt_stats st{};
            check(mi355pt_render_aov(r_.args.scene->raw(), &r_.args.camera->raw(), &p, r_.aov, r_.args.scene->d65_lut(), pixels_.data(), &st), "mi355pt_render_aov");
            return st.kernel_ms * 1e-3;
        }
        if (r_.args.scene->multi()) {                       // several GPUs from this one call: no per-launch statistics
            check(mi355pt_render_multi(r_.args.scene->raw(), &r_.args.camera->raw(), &p, pixels_.data()), "mi355pt_render_multi");
            return 0.0;
        }
        mi355pt_stats st{};
        check(mi355pt_render(r_.args.scene->raw(), &r_.args.camera->raw(), &p, pixels_.data(), &st), "mi355pt_render");
        return st.kernel_ms * 1e-3;
    }
    const std::vector<float>& pixels() const { return pixels_; }
    std::vector<float>& pixels_mut() { return pixels_; }      // for a caller that fills the frame itself (the CLI's --denoise path)
    // RendererImage::save (renderer.rs:137-148): (p*255.0) as u8, PNG
    void save(const std::string& path) const;
private:
    std::vector<float> pixels_; uint32_t w_, h_; SrgbRenderer r_;
};

// ------------------------------------------------------------------ minimal PNG writer (stored deflate blocks, no zlib dependency)
inline uint32_t crc32_of(const uint8_t* d, size_t n, uint32_t crc = 0) {
    static uint32_t table[256]; static bool init = false;
    if (!init) { for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1; table[i] = c; } init = true; }
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ d[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}
inline void write_png_rgb8(const std::string& path, const uint8_t* rgb, uint32_t w, uint32_t h) {
    std::vector<uint8_t> raw; raw.reserve((size_t)(w * 3 + 1) * h);
    for (uint32_t y = 0; y < h; ++y) { raw.push_back(0); raw.insert(raw.end(), rgb + (size_t)y * w * 3, rgb + (size_t)(y + 1) * w * 3); }
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0;
    for (uint8_t c : raw) { a = (a + c) % 65521; b = (b + a) % 65521; }
    for (size_t off = 0; off < raw.size(); off += 65535) {
        size_t n = std::min<size_t>(65535, raw.size() - off);
        z.push_back(off + n == raw.size() ? 1 : 0);
        z.push_back(n & 0xff); z.push_back((n >> 8) & 0xff); z.push_back(~n & 0xff); z.push_back((~n >> 8) & 0xff);
        z.insert(z.end(), raw.begin() + (std::ptrdiff_t)off, raw.begin() + (std::ptrdiff_t)(off + n));
    }
    uint32_t adler = (b << 16) | a;
    for (int i = 3; i >= 0; --i) z.push_back((adler >> (8 * i)) & 0xff);
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    auto be32 = [](uint32_t v, uint8_t* o) { o[0] = v >> 24; o[1] = (v >> 16) & 0xff; o[2] = (v >> 8) & 0xff; o[3] = v & 0xff; };
    auto chunk = [&](const char* tag, const std::vector<uint8_t>& data) {
        uint8_t len[4]; be32((uint32_t)data.size(), len); f.write((char*)len, 4);
        std::vector<uint8_t> td(tag, tag + 4); td.insert(td.end(), data.begin(), data.end());
        f.write((char*)td.data(), (std::streamsize)td.size());
        uint8_t crc[4]; be32(crc32_of(td.data(), td.size()), crc); f.write((char*)crc, 4);
    };
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    f.write((const char*)sig, 8);
    std::vector<uint8_t> ihdr(13); be32(w, &ihdr[0]); be32(h, &ihdr[4]); ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    chunk("IHDR", ihdr); chunk("IDAT", z); chunk("IEND", {});
}
inline void RendererImage::save(const std::string& path) const {
    std::vector<uint8_t> q(pixels_.size());
    check(mi355pt_quantize_u8(pixels_.data(), pixels_.size(), q.data()), "mi355pt_quantize_u8");
    write_png_rgb8(path, q.data(), w_, h_);
}

}  // namespace renderer
