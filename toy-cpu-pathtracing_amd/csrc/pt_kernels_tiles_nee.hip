// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the NEE renderer with the ZSobol sampler: the feature sets without the clearcoat
// code, with the backend options of pt_kernels_nee.hip (Makefile).
#include "pt_kernel_tiles.hpp"
namespace pt {
void launch_pt_tiles_nee_sobol(const PtLaunchArgs& a, uint32_t feat) {
    if (pick_features(feat) & FEAT_CC) launch_pt_tiles_nee_sobol_cc(a, feat); else launch_pt_tiles_plain<MODE_NEE_SOBOL>(a, feat);
}
}  // namespace pt
