// Host driver of tests/test_launch_plan.py: csrc/launch_plan.hpp compiled with plain g++, no HIP.  Reads cases
//   w h spp sampler shard_index shard_count s_begin s_end waves aov
// from stdin; prints per case "case <tiles of the shard>" and, for each launch of the sample range, "r <begin> <end> <plan fields>".
#include <cstdio>

#include "launch_plan.hpp"

int main() {
    mi355pt_camera cam{};
    mi355pt_params p{};
    unsigned s_begin, s_end, aov;
    int waves;
    while (std::scanf("%u %u %u %u %u %u %u %u %d %u", &cam.width, &cam.height, &p.spp, &p.sampler, &p.shard_index, &p.shard_count, &s_begin, &s_end,
                      &waves, &aov) == 10) {
        std::printf("case %u\n", pt::shard_tile_count(cam.width, cam.height, p.shard_index, p.shard_count));
        pt::for_each_launch_range(p.sampler, false, s_begin, s_end, [&](uint32_t b, uint32_t e) {
            const pt::LaunchPlan pl = pt::plan_launch(&cam, &p, b, e, waves, aov != 0);
            const pt::DevParams& d = pl.params;
            std::printf("r %u %u %u %u %u %u %u %u %u %u %u %u %u %d %zu\n", b, e, d.sample_begin, d.sample_end, d.log2_spp, d.n_base4_digits, d.block_log2,
                        d.chunks, d.chunk_size, d.n_work, d.sample_prefix_digits, d.tiles_x * d.tiles_y, pl.n_tiles, pl.grid, pl.partial_floats);
            return 0;
        });
    }
    return 0;
}
