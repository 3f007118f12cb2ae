// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the NEE renderer with the ZSobol sampler: the feature sets without the clearcoat
// code, with the backend options of pt_kernels_nee.hip (Makefile).
#include "pt_kernel_tiles.hpp"
PT_KERNELS_TILES_PLAIN(MODE_NEE_SOBOL)
