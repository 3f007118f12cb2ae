// pt_kernel_tiles (pt_kernel_tiles.hpp), NEE + ZSobol: the feature sets with the clearcoat code, with the backend options of
// pt_kernels_nee_cc.hip (Makefile).
#include "pt_kernel_tiles.hpp"
namespace pt {
void launch_pt_tiles_nee_sobol_cc(const PtLaunchArgs& a, uint32_t feat) { launch_pt_tiles_cc<MODE_NEE_SOBOL>(a, feat); }
}  // namespace pt
