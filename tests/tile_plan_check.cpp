// Host driver of tests/test_tile_plan.py: csrc/launch_plan.hpp compiled with plain g++, no HIP.  Reads cases
//   w h spp sampler s_begin s_end waves n_list
// from stdin; for each launch of the sample range prints "l <begin> <end> <plan fields>" for plan_launch_tiles over n_list tiles and
// "f <begin> <end> <plan fields>" for plan_launch's whole-frame plan (shard 0 of 1), preceded by "case <tiles of the frame>".
#include <cstdio>

#include "launch_plan.hpp"

static void print_plan(char tag, uint32_t b, uint32_t e, const pt::LaunchPlan& pl) {
    const pt::DevParams& d = pl.params;
    std::printf("%c %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %zu\n", tag, b, e, d.spp, d.seed, d.max_depth, d.strategy, d.sampler, d.sample_begin,
                d.sample_end, d.log2_spp, d.n_base4_digits, d.tiles_x, d.tiles_y, d.block_log2, d.chunks, d.chunk_size, d.n_work, d.sample_prefix_digits,
                pl.n_tiles, pl.grid, pl.partial_floats);
}

int main() {
    mi355pt_camera cam{};
    mi355pt_params p{};
    p.shard_count = 1; p.strategy = MI355PT_STRATEGY_MIS; p.max_depth = 16; p.seed = 7;
    unsigned s_begin, s_end, n_list;
    int waves;
    while (std::scanf("%u %u %u %u %u %u %d %u", &cam.width, &cam.height, &p.spp, &p.sampler, &s_begin, &s_end, &waves, &n_list) == 8) {
        std::printf("case %u\n", pt::shard_tile_count(cam.width, cam.height, 0, 1));
        pt::for_each_launch_range(p.sampler, false, s_begin, s_end, [&](uint32_t b, uint32_t e) {
            print_plan('l', b, e, pt::plan_launch_tiles(&cam, &p, b, e, waves, n_list));
            print_plan('f', b, e, pt::plan_launch(&cam, &p, b, e, waves, false));
            return 0;
        });
    }
    return 0;
}
