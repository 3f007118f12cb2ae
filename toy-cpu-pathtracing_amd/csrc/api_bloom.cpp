// The mi355pt_bloom.h surface of libmi355pt.so: the defaults, the scratch size, the refusals and the two entry points of the bloom stage.
// Host C++ only, like api.cpp; the kernels are in pt_kernels_bloom.hip, the shapes in bloom_plan.hpp, the checks in bloom_checks.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/mi355pt_bloom.h"
#include "api_internal.hpp"
#include "bloom_checks.hpp"
#include "bloom_plan.hpp"

using namespace pt;

namespace {

static_assert(sizeof(mi355pt_bloom_params) == 32, "eight 32-bit fields, no padding");
static_assert(MI355PT_BLOOM_MAX_LEVELS == BLOOM_MAX_LEVELS, "the header and the plan agree on the levels");

// the verdict of bloom_checks.hpp as the call's return code and message
int bloom_check(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* bp, const uint32_t* record, const void* scratch,
                size_t scratch_bytes, const float* out, bool device) {
    const char* text = nullptr;
    switch (bloom_verdict(film, width, height, spp, bp, record, scratch, scratch_bytes, out, device)) {
        case Bloom::OK: return MI355PT_OK;
        case Bloom::NULL_POINTER: text = "null params, film, scratch or output pointer"; break;
        case Bloom::SPP_ZERO: text = "spp must be > 0"; break;
        case Bloom::EMPTY_FRAME: text = "zero width or height"; break;
        case Bloom::FRAME_TOO_LARGE: text = "frame too large (width and height up to 2^24, fewer than 2^32 pixels)"; break;
        case Bloom::LEVELS: text = "levels must be in [1, 8] (mi355pt_bloom_params_default fills the struct)"; break;
        case Bloom::FIREFLY: text = "firefly must be 0 or 1"; break;
        case Bloom::THRESHOLD: text = "threshold must be in [0, 2^16]"; break;
        case Bloom::KNEE: text = "knee must be in [0, 1]"; break;
        case Bloom::SCATTER: text = "scatter must be in [0, 1]"; break;
        case Bloom::BASE: text = "base must be in [0, 1]"; break;
        case Bloom::INTENSITY: text = "intensity must be in [0, 16]"; break;
        case Bloom::EXPOSURE: text = "exposure must be finite and > 0"; break;
        case Bloom::SCRATCH_TOO_SMALL: text = "scratch buffer too small (mi355pt_bloom_scratch_bytes gives the size)"; break;
        case Bloom::MISALIGNED: text = "the scratch buffer must be 16-byte aligned and the record 4-byte aligned"; break;
        case Bloom::OVERLAP: text = "the film, the output, the scratch buffer and the record must not overlap (the output may be the film itself)"; break;
    }
    return fail(MI355PT_E_INVALID, std::string("bloom: ") + text);
}

}  // namespace

extern "C" {

void mi355pt_bloom_params_default(mi355pt_bloom_params* out) {
    if (!out) return;
    out->levels = 6; out->firefly = 1;
    out->threshold = 0.0f; out->knee = 0.5f; out->scatter = 0.7f;
    out->intensity = 0.04f; out->base = 1.0f - out->intensity;
    out->exposure = 1.0f;
}

size_t mi355pt_bloom_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels) { return bloom_scratch_bytes(width, height, levels); }

int mi355pt_bloom_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* bp, const uint32_t* d_record, void* d_scratch,
                         size_t scratch_bytes, float* d_out, void* hip_stream) {
    int rc = bloom_check(d_film, width, height, spp, bp, d_record, d_scratch, scratch_bytes, d_out, true);
    if (rc) return rc;
    BloomArgs a{};
    a.width = width; a.height = height; a.levels = bp->levels; a.firefly = bp->firefly;
    a.spp = (float)spp;
    a.threshold = bp->threshold; a.knee = bp->knee; a.exposure = bp->exposure;
    a.s1 = bp->scatter; a.s0 = 1.0f - bp->scatter;
    a.base = bp->base; a.intensity = bp->intensity;
    HIP_TRY(launch_bloom(d_film, a, d_record, d_scratch, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_bloom(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* bp, const uint32_t* record, float* out) {
    int rc = bloom_check(film, width, height, spp, bp, record, nullptr, 0, out, false);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3, scratch_bytes = bloom_scratch_bytes(width, height, bp->levels);
    DevBuf<float> d_film;
    DevBuf<uint32_t> d_record;
    DevBuf<unsigned char> d_scratch;
    HIP_TRY(d_film.upload(film, n));
    HIP_TRY(d_record.upload(record, 8));
    HIP_TRY(d_scratch.alloc(scratch_bytes));
    if ((rc = mi355pt_bloom_device(d_film.p, width, height, spp, bp, d_record.p, d_scratch.p, scratch_bytes, d_film.p, nullptr))) return rc;      // in place, as the header allows
    HIP_TRY(d_film.download(out, n));
    return MI355PT_OK;
}

}  // extern "C"
