// The mi355pt_display.h surface of libmi355pt.so: the defaults, the scratch size, the argument checks and the four entry points of the display
// stage.  Host C++ only, like api.cpp; the kernels are in pt_kernels_display.hip, the shape of the meter's first launch in display_plan.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mi355pt_debug.h"
#include "api_internal.hpp"
#include "display_plan.hpp"

using namespace pt;

namespace {

constexpr size_t RECORD_BYTES = MI355PT_DISPLAY_RECORD_WORDS * sizeof(uint32_t), HIST_BYTES = MI355PT_DISPLAY_HIST_WORDS * sizeof(uint32_t);
static_assert(MI355PT_DISPLAY_HIST_WORDS == DISPLAY_HIST_WORDS, "the header and the plan agree on the histogram");

// the checks of a params struct, shared by the meter and the display: the struct is valid or refused as a whole
int params_check(const mi355pt_display_params* dp, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (dp->tone > MI355PT_TONE_HABLE) return fail(MI355PT_E_INVALID, w + "unknown tone operator");
    if (dp->encode > MI355PT_ENCODE_SRGB) return fail(MI355PT_E_INVALID, w + "unknown encoding");
    if (!all_finite_positive({dp->exposure})) return fail(MI355PT_E_INVALID, w + "exposure must be finite and > 0 (mi355pt_display_params_default fills the struct)");
    if (!std::isfinite(dp->white) || !(dp->white >= 0x1p-16f && dp->white <= 0x1p16f)) return fail(MI355PT_E_INVALID, w + "white must be in [2^-16, 2^16]");
    if (dp->log2_lum_min < -126 || dp->log2_lum_min > 95) return fail(MI355PT_E_INVALID, w + "log2_lum_min must be in [-126, 95]: every bin edge is a normal float");
    if ((uint64_t)dp->trim_low + dp->trim_high >= 1024u) return fail(MI355PT_E_INVALID, w + "trim_low + trim_high must be below 1024 (they are 1/1024ths)");
    if (!all_finite_positive({dp->key, dp->e_min, dp->e_max})) return fail(MI355PT_E_INVALID, w + "key, e_min and e_max must be finite and > 0");
    if (dp->e_min > dp->e_max) return fail(MI355PT_E_INVALID, w + "e_min is above e_max");
    if (!(dp->adapt >= 0.0f && dp->adapt <= 1.0f)) return fail(MI355PT_E_INVALID, w + "adapt must be in [0, 1]");
    return MI355PT_OK;
}

int frame_check(uint32_t width, uint32_t height, uint32_t spp, const char* who) {
    const std::string w = std::string(who) + ": ";
    if (spp == 0) return fail(MI355PT_E_INVALID, w + "spp must be > 0");
    if (width == 0 || height == 0) return fail(MI355PT_E_INVALID, w + "zero width or height");
    if (plan_display_meter(width, height).rows == 0) return fail(MI355PT_E_INVALID, w + "frame too large (width and height up to 2^24, fewer than 2^32 pixels)");
    return MI355PT_OK;
}

// every check of mi355pt_display_meter_device / mi355pt_display_meter (`device`: the scratch buffer is the caller's); host arithmetic only
int meter_check(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* prev, const void* scratch,
                size_t scratch_bytes, const uint32_t* record, const uint32_t* hist, bool device) {
    const char* who = "display meter";
    if (!dp || !film || !record || (device && !scratch)) return fail(MI355PT_E_INVALID, "display meter: null params, film, scratch or record pointer");
    int rc = frame_check(width, height, spp, who);
    if (rc) return rc;
    const size_t need = display_scratch_bytes(width, height), film_bytes = (size_t)width * height * 3 * sizeof(float);
    if (device && scratch_bytes < need) return fail(MI355PT_E_INVALID, "display meter: scratch buffer too small (mi355pt_display_scratch_bytes gives the size)");
    if (misaligned(scratch, 4) || misaligned(record, 4) || misaligned(prev, 4) || misaligned(hist, 4)) return fail(MI355PT_E_INVALID, "display meter: the scratch buffer, the records and the histogram must be 4-byte aligned");
    rc = params_check(dp, who);
    if (rc) return rc;
    const void* outs[2] = {record, hist};
    const size_t out_bytes[2] = {RECORD_BYTES, HIST_BYTES};
    for (int i = 0; i < 2; ++i)
        if (overlap(outs[i], out_bytes[i], film, film_bytes) || (device && overlap(outs[i], out_bytes[i], scratch, need)))
            return fail(MI355PT_E_INVALID, "display meter: an output overlaps the film or the scratch buffer");
    if (overlap(hist, HIST_BYTES, record, RECORD_BYTES) || overlap(hist, HIST_BYTES, prev, RECORD_BYTES)) return fail(MI355PT_E_INVALID, "display meter: the histogram overlaps a record");
    if (overlap(prev, RECORD_BYTES, film, film_bytes) || (device && overlap(prev, RECORD_BYTES, scratch, need)))
        return fail(MI355PT_E_INVALID, "display meter: the previous record overlaps the film or the scratch buffer");
    if (prev != record && overlap(prev, RECORD_BYTES, record, RECORD_BYTES)) return fail(MI355PT_E_INVALID, "display meter: the previous record overlaps the record without being it");
    return MI355PT_OK;
}

int display_check(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* record, const float* out) {
    const char* who = "display";
    if (!dp || !film || !out) return fail(MI355PT_E_INVALID, "display: null params, film or output pointer");
    int rc = frame_check(width, height, spp, who);
    if (rc) return rc;
    if (misaligned(record, 4)) return fail(MI355PT_E_INVALID, "display: the record must be 4-byte aligned");
    rc = params_check(dp, who);
    if (rc) return rc;
    const size_t film_bytes = (size_t)width * height * 3 * sizeof(float);
    if (overlap(out, film_bytes, film, film_bytes) || overlap(out, film_bytes, record, RECORD_BYTES)) return fail(MI355PT_E_INVALID, "display: the output overlaps the film or the record");
    return MI355PT_OK;
}

DisplayMeterArgs meter_args(uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp) {
    DisplayMeterArgs a{};
    a.width = width; a.height = height; a.spp = (float)spp;
    a.base = (uint32_t)(dp->log2_lum_min + 127) << 3;
    a.trim_low = dp->trim_low; a.trim_high = dp->trim_high;
    a.key = dp->key; a.e_min = dp->e_min; a.e_max = dp->e_max; a.adapt = dp->adapt;
    return a;
}

}  // namespace

extern "C" {

void mi355pt_display_params_default(mi355pt_display_params* out) {
    if (!out) return;
    out->tone = MI355PT_TONE_REINHARD; out->encode = MI355PT_ENCODE_SRGB;
    out->exposure = 1.0f; out->white = 11.2f;
    out->log2_lum_min = -16; out->trim_low = 102; out->trim_high = 51;
    out->key = 0.18f; out->e_min = 0x1p-10f; out->e_max = 0x1p10f; out->adapt = 1.0f;
}

size_t mi355pt_display_scratch_bytes(uint32_t width, uint32_t height) { return display_scratch_bytes(width, height); }

int mi355pt_display_meter_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* d_prev_record,
                                 void* d_scratch, size_t scratch_bytes, uint32_t* d_record, uint32_t* d_hist, void* hip_stream) {
    int rc = meter_check(d_film, width, height, spp, dp, d_prev_record, d_scratch, scratch_bytes, d_record, d_hist, true);
    if (rc) return rc;
    const DisplayMeterArgs a = meter_args(width, height, spp, dp);
    HIP_TRY(launch_display_meter(d_film, a, d_prev_record, (uint32_t*)d_scratch, d_record, d_hist, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_display_device(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* d_record,
                           float* d_out, void* hip_stream) {
    int rc = display_check(d_film, width, height, spp, dp, d_record, d_out);
    if (rc) return rc;
    DisplayArgs a{};
    a.width = width; a.height = height; a.spp = (float)spp;
    a.tone = dp->tone; a.encode = dp->encode; a.exposure = dp->exposure;
    a.white2 = dp->white * dp->white;
    a.hable_white = display_hable(dp->white);
    HIP_TRY(launch_display(d_film, a, d_record, d_out, (hipStream_t)hip_stream));
    return MI355PT_OK;
}

int mi355pt_display_meter(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* prev_record,
                          uint32_t* record, uint32_t* hist) {
    int rc = meter_check(film, width, height, spp, dp, prev_record, nullptr, 0, record, hist, false);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3, scratch_bytes = display_scratch_bytes(width, height);
    DevBuf<float> d_film;
    DevBuf<uint32_t> d_scratch, d_record, d_hist;
    HIP_TRY(d_film.upload(film, n));
    HIP_TRY(d_scratch.alloc(scratch_bytes / sizeof(uint32_t)));
    HIP_TRY(prev_record ? d_record.upload(prev_record, MI355PT_DISPLAY_RECORD_WORDS) : d_record.alloc(MI355PT_DISPLAY_RECORD_WORDS));      // metered in place, as the header allows
    HIP_TRY(d_hist.alloc_for(hist, MI355PT_DISPLAY_HIST_WORDS));
    if ((rc = mi355pt_display_meter_device(d_film.p, width, height, spp, dp, prev_record ? d_record.p : nullptr, d_scratch.p, scratch_bytes, d_record.p, d_hist.p,
                                           nullptr))) return rc;
    HIP_TRY(d_record.download(record, MI355PT_DISPLAY_RECORD_WORDS));
    HIP_TRY(d_hist.download(hist, MI355PT_DISPLAY_HIST_WORDS));
    return MI355PT_OK;
}

int mi355pt_display(const float* film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, const uint32_t* record, float* out) {
    int rc = display_check(film, width, height, spp, dp, record, out);
    if (rc) return rc;
    const size_t n = (size_t)width * height * 3;
    DevBuf<float> d_film, d_out;
    DevBuf<uint32_t> d_record;
    HIP_TRY(d_film.upload(film, n));
    HIP_TRY(d_record.upload(record, MI355PT_DISPLAY_RECORD_WORDS));
    HIP_TRY(d_out.alloc(n));
    if ((rc = mi355pt_display_device(d_film.p, width, height, spp, dp, d_record.p, d_out.p, nullptr))) return rc;
    HIP_TRY(d_out.download(out, n));
    return MI355PT_OK;
}

// include/mi355pt_debug.h: the meter's two launches with an event between them (tools/display_rate.py).  Synchronises.
int mi355pt_probe_display_meter_ms(const float* d_film, uint32_t width, uint32_t height, uint32_t spp, const mi355pt_display_params* dp, void* d_scratch,
                                   size_t scratch_bytes, uint32_t* d_record, float* out_ms) {
    if (!out_ms) return fail(MI355PT_E_INVALID, "display meter probe: null output");
    int rc = meter_check(d_film, width, height, spp, dp, nullptr, d_scratch, scratch_bytes, d_record, nullptr, true);
    if (rc) return rc;
    const DisplayMeterArgs a = meter_args(width, height, spp, dp);
    Event ev[3];
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = ev[i].create();
    if (e == hipSuccess) e = ev[0].record(nullptr);
    if (e == hipSuccess) e = launch_display_hist(d_film, a, (uint32_t*)d_scratch, nullptr);
    if (e == hipSuccess) e = ev[1].record(nullptr);
    if (e == hipSuccess) e = launch_display_finish((const uint32_t*)d_scratch, a, nullptr, d_record, nullptr, nullptr);
    if (e == hipSuccess) e = ev[2].record(nullptr);
    if (e == hipSuccess) e = ev[2].synchronize();
    if (e == hipSuccess) e = ev[1].elapsed_ms(ev[0], &out_ms[0]);
    if (e == hipSuccess) e = ev[2].elapsed_ms(ev[1], &out_ms[1]);
    if (e != hipSuccess) return fail(MI355PT_E_DEVICE, std::string("display meter probe: ") + hipGetErrorString(e));
    return MI355PT_OK;
}

}  // extern "C"
