// Host driver of tests/test_film_log.py: the f32 XYZ -> sRGB matrices the sensor is evaluated with, compiled with plain g++, no HIP.
// Prints "product" and the nine floats of csrc/launch_plan.hpp srgb_xyz_to_rgb (row-major: DevParams.xyz_to_rgb, what film_rgb multiplies
// with), then "oracle" and the oracle's (oracle/o_spectrum.hpp, m[col][row]) in the same row-major order; every float with 9 digits.
#include <cstdio>

#include "launch_plan.hpp"
#include "o_spectrum.hpp"

int main() {
    float p[9];
    pt::srgb_xyz_to_rgb(p);
    std::printf("product");
    for (float v : p) std::printf(" %.9g", v);
    const oracle::M3 o = oracle::srgb_xyz_to_rgb();
    std::printf("\noracle");
    for (int row = 0; row < 3; ++row) for (int col = 0; col < 3; ++col) std::printf(" %.9g", o.m[col][row]);
    std::printf("\n");
    return 0;
}
