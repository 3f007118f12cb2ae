// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the MIS renderer with the ZSobol sampler: the feature sets without the clearcoat
// code, with the backend options of pt_kernels_mis.hip (Makefile).
#include "pt_kernel_tiles.hpp"
PT_KERNELS_TILES_PLAIN(MODE_MIS_SOBOL)
