// Host driver of tests/test_bloom.py: csrc/bloom_checks.hpp compiled with plain g++, no HIP, no library.  Reads one case per line from stdin,
//   device film out scratch record scratch_bytes width height spp has_params levels firefly threshold knee scatter base intensity exposure
// — the four buffers as addresses (0: a null pointer; nothing is dereferenced), the six floats of the params struct as the u32 bit patterns
// of their binary32 values — and prints the name of bloom_verdict's answer.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "bloom_checks.hpp"

int main() {
    unsigned device, has_params, width, height, spp, levels, firefly, f[6];
    uint64_t film, out, scratch, record, scratch_bytes;
    while (std::scanf("%u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %u %u %u %u %u %u %u %u %u %u %u %u", &device, &film, &out, &scratch, &record, &scratch_bytes,
                      &width, &height, &spp, &has_params, &levels, &firefly, &f[0], &f[1], &f[2], &f[3], &f[4], &f[5]) == 18) {
        mi355pt_bloom_params p;
        p.levels = levels; p.firefly = firefly;
        float v[6];
        std::memcpy(v, f, sizeof v);
        p.threshold = v[0]; p.knee = v[1]; p.scatter = v[2]; p.base = v[3]; p.intensity = v[4]; p.exposure = v[5];
        const pt::Bloom verdict = pt::bloom_verdict((const void*)(uintptr_t)film, width, height, spp, has_params ? &p : nullptr, (const void*)(uintptr_t)record,
                                                    (const void*)(uintptr_t)scratch, (size_t)scratch_bytes, (const void*)(uintptr_t)out, device != 0);
        std::printf("%s\n", pt::bloom_verdict_name(verdict));
    }
    return 0;
}
