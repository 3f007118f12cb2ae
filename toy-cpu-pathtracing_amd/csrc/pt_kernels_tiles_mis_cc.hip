// pt_kernel_tiles (pt_kernel_tiles.hpp), MIS + ZSobol: the feature sets with the clearcoat code, with the backend options of
// pt_kernels_mis_cc.hip (Makefile).
#include "pt_kernel_tiles.hpp"
PT_KERNELS_TILES_CC(MODE_MIS_SOBOL)
