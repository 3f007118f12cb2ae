// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the MIS renderer with the ZSobol sampler: the feature sets without the clearcoat
// code, with the backend options of pt_kernels_mis.hip (Makefile).
#include "pt_kernel_tiles.hpp"
namespace pt {
void launch_pt_tiles_mis_sobol(const PtLaunchArgs& a, uint32_t feat) {
    if (pick_features(feat) & FEAT_CC) launch_pt_tiles_mis_sobol_cc(a, feat); else launch_pt_tiles_plain<MODE_MIS_SOBOL>(a, feat);
}
}  // namespace pt
