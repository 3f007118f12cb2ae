// The shape of the bloom stage (include/mi355pt_bloom.h) as pure arithmetic, in the manner of display_plan.hpp: no HIP, one text for the host
// (api_bloom.cpp, the launchers) and for the kernels (pt_kernels_bloom.hip takes the tile constants), compiled with plain g++ by
// tests/test_bloom.py (tests/bloom_plan_check.cpp).  Level l = 0 is the frame; level l = 1 .. L is ((W_{l-1} + 1) >> 1) x ((H_{l-1} + 1) >> 1)
// records of 16 bytes in the scratch buffer, level after level.
//
// The reduction (bloom_down_kernel) makes BLOOM_TX x BLOOM_TY destination pixels per workgroup of 256 threads and stages the
// BLOOM_SRC_W x BLOOM_SRC_H source texels they read, one plane of floats per channel.  BLOOM_TX = 32: a 32-lane half of a wave is then ONE row
// of the tile in all three LDS phases, and the LDS conflict rules hold within a half at most (MI355X: 4-byte accesses are served per 32
// lanes over 32 banks, consecutive floats; the horizontal pass takes its four texels as two 8-byte reads, which the compiler pairs into one
// ds_read2_b64, served per 16 lanes over 32 banks: lane i reads dwords 2 i and 2 i + 1, then 2 i + 2 and 2 i + 3 — 32 distinct banks each
// time) — so no choice of row pitch can make two rows collide, and the pitch is simply the staged width, which is even, as the 8-byte
// reads need.
// The expansion (bloom_up_kernel) is one thread per destination pixel in blocks of BLOOM_UP_X x BLOOM_UP_Y.
// Both grids are one-dimensional (tiles_x * tiles_y blocks): a 1 x 2^24 frame has more rows of tiles than a grid's y extent allows.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pt {

constexpr uint32_t BLOOM_MAX_LEVELS = 8;
constexpr uint32_t BLOOM_TX = 32, BLOOM_TY = 8;                        // destination pixels of a reduction's workgroup
constexpr uint32_t BLOOM_DOWN_BLOCK = BLOOM_TX * BLOOM_TY;             // its threads: four waves
constexpr uint32_t BLOOM_SRC_W = 2 * BLOOM_TX + 2, BLOOM_SRC_H = 2 * BLOOM_TY + 2;   // the source texels it stages
constexpr uint32_t BLOOM_SRC_PITCH = BLOOM_SRC_W;                      // floats per staged row (even: the horizontal pass reads 8 bytes)
constexpr uint32_t BLOOM_UP_X = 64, BLOOM_UP_Y = 4;                    // destination pixels of an expansion's workgroup, one per thread
constexpr uint32_t BLOOM_RECORD_BYTES = 16;
static_assert(BLOOM_SRC_PITCH % 2 == 0 && BLOOM_TX == 32, "see above");

struct BloomLevel {
    uint32_t width = 0, height = 0;
    uint64_t offset = 0;            // in RECORDS from the start of the scratch buffer (level 0: not in the buffer, 0)
    uint32_t down_blocks = 0;       // grid of the reduction that WRITES this level (level 0: none, 0)
    uint32_t up_blocks = 0;         // grid of the expansion that writes this level's size: U_l for l >= 1, the composite for l = 0 (level L: none, 0)
};
struct BloomPlan {
    uint32_t levels = 0;            // 0: a call the stage refuses
    uint64_t records = 0;           // of the whole scratch buffer
    BloomLevel level[BLOOM_MAX_LEVELS + 1];
};

constexpr uint32_t bloom_blocks(uint32_t width, uint32_t height, uint32_t bx, uint32_t by) {
    return (uint32_t)((uint64_t)((width + bx - 1) / bx) * ((height + by - 1) / by));
}

// width and height 1 .. 2^24, fewer than 2^32 pixels and 1 .. 8 levels, or an all-zero plan
inline BloomPlan plan_bloom(uint32_t width, uint32_t height, uint32_t levels) {
    BloomPlan p;
    if (width == 0 || height == 0 || width > (1u << 24) || height > (1u << 24) || levels == 0 || levels > BLOOM_MAX_LEVELS) return p;
    if (((uint64_t)width * height) >> 32) return p;
    p.levels = levels;
    p.level[0].width = width; p.level[0].height = height;
    for (uint32_t l = 1; l <= levels; ++l) {
        BloomLevel& v = p.level[l];
        v.width = (p.level[l - 1].width + 1) >> 1; v.height = (p.level[l - 1].height + 1) >> 1;
        v.offset = p.records;
        p.records += (uint64_t)v.width * v.height;
        v.down_blocks = bloom_blocks(v.width, v.height, BLOOM_TX, BLOOM_TY);
    }
    for (uint32_t l = 0; l < levels; ++l) p.level[l].up_blocks = bloom_blocks(p.level[l].width, p.level[l].height, BLOOM_UP_X, BLOOM_UP_Y);
    return p;
}

inline size_t bloom_scratch_bytes(uint32_t width, uint32_t height, uint32_t levels) {
    return (size_t)(plan_bloom(width, height, levels).records * BLOOM_RECORD_BYTES);
}

}  // namespace pt
