// pt_kernel specialised for the NEE renderer with the ZSobol sampler (C5): the feature sets with the clearcoat code (3 waves per SIMD).
#include "pt_kernel.hpp"
PT_KERNELS_CC(MODE_NEE_SOBOL)
