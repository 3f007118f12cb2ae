// Host driver of tests/test_display.py: csrc/display_plan.hpp compiled with plain g++, no HIP.  Reads cases "width height" from stdin and
// prints per case "pixels chunks rows trips scratch_bytes covered twice": `covered` counts the pixels that the blocks' trips reach, `twice`
// those reached more than once.  Frames of up to 2^22 pixels are walked pixel by pixel, exactly as the kernel indexes them; larger ones chunk
// by chunk (a chunk's pixels are consecutive, so a chunk is reached as a whole or not at all).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "display_plan.hpp"

int main() {
    unsigned w, h;
    while (std::scanf("%u %u", &w, &h) == 2) {
        const pt::DisplayMeterPlan p = pt::plan_display_meter(w, h);
        uint64_t covered = 0, twice = 0;
        if (p.rows != 0 && p.pixels <= (1ull << 22)) {
            std::vector<uint8_t> seen(p.pixels, 0);
            for (uint32_t b = 0; b < p.rows; ++b)
                for (uint32_t k = 0; k < p.trips; ++k)
                    for (uint32_t t = 0; t < pt::DISPLAY_METER_BLOCK; ++t) {
                        const uint64_t i = ((uint64_t)k * p.rows + b) * pt::DISPLAY_METER_BLOCK + t;      // display_hist_kernel's index
                        if (i >= p.pixels) continue;
                        if (seen[i]++) ++twice; else ++covered;
                    }
        } else if (p.rows != 0) {
            std::vector<uint8_t> seen(p.chunks, 0);
            for (uint32_t b = 0; b < p.rows; ++b)
                for (uint32_t k = 0; k < p.trips; ++k) {
                    const uint64_t c = (uint64_t)k * p.rows + b;
                    if (c >= p.chunks) continue;
                    const uint64_t first = c * pt::DISPLAY_METER_BLOCK, last = first + pt::DISPLAY_METER_BLOCK < p.pixels ? first + pt::DISPLAY_METER_BLOCK : p.pixels;
                    if (seen[c]++) twice += last - first; else covered += last - first;
                }
        }
        std::printf("%llu %llu %u %u %zu %llu %llu\n", (unsigned long long)p.pixels, (unsigned long long)p.chunks, p.rows, p.trips, pt::display_scratch_bytes(w, h),
                    (unsigned long long)covered, (unsigned long long)twice);
    }
    return 0;
}
