// The shape of the display meter's first launch (include/mi355pt_display.h) as pure host arithmetic, in the manner of launch_plan.hpp: no
// HIP, compiled with plain g++ by tests/test_display.py.  The frame's pixels are taken in CHUNKS of DISPLAY_METER_BLOCK consecutive pixels;
// block b of `rows` takes the chunks b, b + rows, b + 2 rows, ... in `trips` trips through its grid-stride loop, and stores its 258 partial
// counts as row b of the scratch buffer.  rows is capped: the second launch, one block, reads rows x 258 words.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pt {

constexpr uint32_t DISPLAY_METER_BLOCK = 1024;     // threads of a block of the first launch = pixels of a chunk
constexpr uint32_t DISPLAY_METER_MAX_ROWS = 256;   // one block of sixteen waves on each of the MI355X's 256 CUs: as many lanes in flight as 1024 blocks
                                                   // of 256 had, a quarter of the rows for the second launch to sum
constexpr uint32_t DISPLAY_HIST_WORDS = 258;       // 256 bins, below, above
constexpr uint32_t DISPLAY_FINISH_BLOCK = 1024;    // threads of the second launch: four groups of 256, each summing a quarter of the rows; at least 2 x MAX_ROWS

struct DisplayMeterPlan {
    uint64_t pixels = 0;     // width * height; 0: a frame the meter refuses
    uint64_t chunks = 0;     // ceil(pixels / DISPLAY_METER_BLOCK)
    uint32_t rows = 0;       // blocks of the first launch = rows of the scratch buffer: min(chunks, DISPLAY_METER_MAX_ROWS)
    uint32_t trips = 0;      // ceil(chunks / rows): every block makes this many trips; in the last one a block may find no chunk
};

// width and height 1 .. 2^24 and fewer than 2^32 pixels, or an all-zero plan
inline DisplayMeterPlan plan_display_meter(uint32_t width, uint32_t height) {
    DisplayMeterPlan p;
    if (width == 0 || height == 0 || width > (1u << 24) || height > (1u << 24)) return p;
    const uint64_t n = (uint64_t)width * height;
    if (n >= (1ull << 32)) return p;
    p.pixels = n;
    p.chunks = (n + DISPLAY_METER_BLOCK - 1) / DISPLAY_METER_BLOCK;
    p.rows = (uint32_t)(p.chunks < DISPLAY_METER_MAX_ROWS ? p.chunks : DISPLAY_METER_MAX_ROWS);
    p.trips = (uint32_t)((p.chunks + p.rows - 1) / p.rows);
    return p;
}

inline size_t display_scratch_bytes(uint32_t width, uint32_t height) {
    return (size_t)plan_display_meter(width, height).rows * DISPLAY_HIST_WORDS * sizeof(uint32_t);
}

}  // namespace pt
