#include "conv_igemm_kernel.h"
template int launch_igemm<bf16, 1, 4>(const ConvArgs&, const IgemmPlan&, hipStream_t);
