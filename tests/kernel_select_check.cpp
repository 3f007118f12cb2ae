// Host driver of tests/test_kernel_select.py: csrc/launch_plan.hpp compiled with plain g++, no HIP.  Prints the list of compiled feature sets
// ("sets ..."), its two classes ("plain ...", "cc ...") and, for every (tiles, stats, feature mask, sampler, strategy),
// "k <tiles> <stats> <feat> <sampler> <strategy> <key.tiles> <key.stats> <key.mode> <key.set>".
#include <cstdio>

#include "launch_plan.hpp"

template <size_t N>
static void print_sets(const char* tag, const uint32_t (&sets)[N]) {
    std::printf("%s", tag);
    for (uint32_t s : sets) std::printf(" %u", s);
    std::printf("\n");
}

int main() {
    print_sets("sets", pt::FEATURE_SETS);
    print_sets("plain", pt::PLAIN_SETS);
    print_sets("cc", pt::CC_SETS);
    std::printf("modes %u %u %u %u\n", pt::MODE_GENERIC, pt::MODE_MIS_SOBOL, pt::MODE_NEE_SOBOL, pt::MODE_PT);
    for (unsigned tiles = 0; tiles < 2; ++tiles)
        for (unsigned stats = 0; stats < 2; ++stats)
            for (uint32_t feat = 0; feat <= pt::FEAT_ALL; ++feat)
                for (uint32_t sampler = 0; sampler < 2; ++sampler)
                    for (uint32_t strategy = 0; strategy < 3; ++strategy) {
                        const pt::KernelKey k = pt::select_kernel(tiles != 0, stats != 0, feat, sampler, strategy);
                        std::printf("k %u %u %u %u %u %d %d %u %u\n", tiles, stats, feat, sampler, strategy, (int)k.tiles, (int)k.stats, k.mode, k.set);
                    }
    return 0;
}
