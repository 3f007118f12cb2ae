// pt_kernel specialised for the MIS renderer with the ZSobol sampler: the feature sets with the clearcoat code (3 waves per SIMD).
#include "pt_kernel.hpp"
PT_KERNELS_CC(MODE_MIS_SOBOL)
