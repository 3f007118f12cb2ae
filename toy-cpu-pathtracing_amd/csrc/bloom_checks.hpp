// The argument checks of the bloom stage (include/mi355pt_bloom.h) as ONE pure predicate in the manner of api_checks.hpp and flow_checks.hpp:
// host arithmetic only, no HIP, nothing is dereferenced but the params struct.  api_bloom.cpp turns the verdict into the refusal's text;
// tests/bloom_checks_check.cpp walks the cases of tests/golden/bloom_refusals.json through it without a library.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mi355pt_bloom.h"
#include "api_checks.hpp"
#include "bloom_plan.hpp"

namespace pt {

// what is wrong with a call: the first that applies, in this order
enum class Bloom { OK, NULL_POINTER, SPP_ZERO, EMPTY_FRAME, FRAME_TOO_LARGE, LEVELS, FIREFLY, THRESHOLD, KNEE, SCATTER, BASE, INTENSITY, EXPOSURE,
                   SCRATCH_TOO_SMALL, MISALIGNED, OVERLAP };

inline const char* bloom_verdict_name(Bloom v) {
    static const char* const names[] = {"OK", "NULL_POINTER", "SPP_ZERO", "EMPTY_FRAME", "FRAME_TOO_LARGE", "LEVELS", "FIREFLY", "THRESHOLD", "KNEE", "SCATTER", "BASE",
                                        "INTENSITY", "EXPOSURE", "SCRATCH_TOO_SMALL", "MISALIGNED", "OVERLAP"};
    return names[(int)v];
}

inline bool bloom_in_range(float v, float lo, float hi) { return v >= lo && v <= hi; }      // false for a NaN

// a params struct is valid or refused as a whole
inline Bloom bloom_params_verdict(const mi355pt_bloom_params& p) {
    if (p.levels < 1u || p.levels > BLOOM_MAX_LEVELS) return Bloom::LEVELS;
    if (p.firefly > 1u) return Bloom::FIREFLY;
    if (!bloom_in_range(p.threshold, 0.0f, 0x1p16f)) return Bloom::THRESHOLD;
    if (!bloom_in_range(p.knee, 0.0f, 1.0f)) return Bloom::KNEE;
    if (!bloom_in_range(p.scatter, 0.0f, 1.0f)) return Bloom::SCATTER;
    if (!bloom_in_range(p.base, 0.0f, 1.0f)) return Bloom::BASE;
    if (!bloom_in_range(p.intensity, 0.0f, 16.0f)) return Bloom::INTENSITY;
    if (!all_finite_positive({p.exposure})) return Bloom::EXPOSURE;
    return Bloom::OK;
}

// `device`: the scratch buffer is the caller's (the host form allocates its own: scratch and scratch_bytes are not looked at)
inline Bloom bloom_verdict(const void* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_bloom_params* params, const void* record, const void* scratch,
                           size_t scratch_bytes, const void* out, bool device) {
    if (!params || !film || !out || (device && !scratch)) return Bloom::NULL_POINTER;
    if (spp == 0u) return Bloom::SPP_ZERO;
    if (width == 0u || height == 0u) return Bloom::EMPTY_FRAME;
    if (frame_too_large(width, height)) return Bloom::FRAME_TOO_LARGE;
    const Bloom pv = bloom_params_verdict(*params);
    if (pv != Bloom::OK) return pv;
    const size_t need = bloom_scratch_bytes(width, height, params->levels), film_bytes = (size_t)width * height * 3 * sizeof(float), record_bytes = 8 * sizeof(uint32_t);
    if (device && scratch_bytes < need) return Bloom::SCRATCH_TOO_SMALL;
    if ((device && misaligned(scratch, 16)) || misaligned(record, 4)) return Bloom::MISALIGNED;
    if (out != film && overlap(out, film_bytes, film, film_bytes)) return Bloom::OVERLAP;
    if (overlap(record, record_bytes, film, film_bytes) || overlap(record, record_bytes, out, film_bytes)) return Bloom::OVERLAP;
    if (device && (overlap(scratch, need, film, film_bytes) || overlap(scratch, need, out, film_bytes) || overlap(scratch, need, record, record_bytes))) return Bloom::OVERLAP;
    return Bloom::OK;
}

}  // namespace pt
