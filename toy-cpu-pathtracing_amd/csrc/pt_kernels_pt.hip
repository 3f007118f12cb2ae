// pt_kernel specialised for the plain path tracer (strategy pt, either sampler: BASELINE configs[0] is pt + random): no light connections
// exist, so these kernels keep the closest-hit traversal alone (pt_kernel.hpp, merged_traversal) and fold the strategy branches away.
// Both feature-set classes in one unit.
#include "pt_kernel.hpp"
PT_KERNELS_CC(MODE_PT)
PT_KERNELS_PLAIN(MODE_PT)
