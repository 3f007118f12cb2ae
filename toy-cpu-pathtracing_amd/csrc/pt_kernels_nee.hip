// pt_kernel specialised for the NEE renderer with the ZSobol sampler: the feature sets without the clearcoat code (C5's kernel is in
// pt_kernels_nee_cc.hip; the two translation units are compiled with different backend options, Makefile).
#include "pt_kernel.hpp"
PT_KERNELS_PLAIN(MODE_NEE_SOBOL)
