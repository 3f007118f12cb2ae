// pt_kernel_tiles (pt_kernel_tiles.hpp), NEE + ZSobol: the feature sets with the clearcoat code, with the backend options of
// pt_kernels_nee_cc.hip (Makefile).
#include "pt_kernel_tiles.hpp"
PT_KERNELS_TILES_CC(MODE_NEE_SOBOL)
