// pt_kernel specialised for the MIS renderer with the ZSobol sampler (every BASELINE config but C1 and C5): the feature sets without the
// clearcoat code (pt_kernels_mis_cc.hip holds the others; the two translation units are compiled with different backend options, Makefile).
#include "pt_kernel.hpp"
PT_KERNELS_PLAIN(MODE_MIS_SOBOL)
