// pt_kernel_tiles (pt_kernel_tiles.hpp) specialised for the plain path tracer (strategy pt, either sampler), like pt_kernels_pt.hip.
#include "pt_kernel_tiles.hpp"
namespace pt {
void launch_pt_tiles_strategy_pt(const PtLaunchArgs& a, uint32_t feat) {
    if (pick_features(feat) & FEAT_CC) launch_pt_tiles_cc<MODE_PT>(a, feat); else launch_pt_tiles_plain<MODE_PT>(a, feat);
}
}  // namespace pt
