// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the plain path tracer (strategy pt, either sampler), like pt_kernels_pt.hip.
#include "pt_kernel_tiles.hpp"
PT_KERNELS_TILES_CC(MODE_PT)
PT_KERNELS_TILES_PLAIN(MODE_PT)
