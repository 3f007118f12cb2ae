// Host driver of tests/test_bloom.py: csrc/bloom_plan.hpp compiled with plain g++, no HIP.  Reads cases "width height levels" from stdin and
// prints per case one line: "levels scratch_bytes TX TY UPX UPY" and then, for l = 0 .. levels, "width height offset down_blocks up_blocks"
// (a refused case prints "0 0 TX TY UPX UPY" alone).
#include <cstdint>
#include <cstdio>

#include "bloom_plan.hpp"

int main() {
    unsigned w, h, levels;
    while (std::scanf("%u %u %u", &w, &h, &levels) == 3) {
        const pt::BloomPlan p = pt::plan_bloom(w, h, levels);
        std::printf("%u %zu %u %u %u %u", p.levels, pt::bloom_scratch_bytes(w, h, levels), pt::BLOOM_TX, pt::BLOOM_TY, pt::BLOOM_UP_X, pt::BLOOM_UP_Y);
        for (uint32_t l = 0; p.levels != 0 && l <= p.levels; ++l)
            std::printf(" %u %u %llu %u %u", p.level[l].width, p.level[l].height, (unsigned long long)p.level[l].offset, p.level[l].down_blocks, p.level[l].up_blocks);
        std::printf("\n");
    }
    return 0;
}
