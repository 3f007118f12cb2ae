// What the two denoiser units (pt_kernels_denoise.hip, pt_kernels_denoise_var.hip) share: the block shape, the B3-spline taps and the
// prepass's cleaning of a film value.  Device helpers only; each unit keeps its own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace pt {

constexpr int DN_BLOCK_X = 64, DN_BLOCK_Y = 4;

// the B3-spline taps h = (1/16, 1/4, 3/8, 1/4, 1/16)
__host__ __device__ constexpr float dn_h5(int k) { return (k == 0 || k == 4) ? 1.0f / 16.0f : ((k == 1 || k == 3) ? 1.0f / 4.0f : 3.0f / 8.0f); }

// c = B / spp, non-finite -> 0, max(c, 0) (NaN and -0 give +0); also a = max(A / spp, 0)
__device__ __forceinline__ float dn_clean(float sum, float spp) {
    const float c = sum / spp;
    return (c > 0.0f && c <= FLT_MAX) ? c : 0.0f;
}
__device__ __forceinline__ float dn_clip0(float sum, float spp) {
    const float a = sum / spp;
    return a > 0.0f ? a : 0.0f;
}

}  // namespace pt
