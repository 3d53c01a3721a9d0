// Fused flagger for median windows of 9, 11 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(9);
KSP_FUSED_INSTANTIATE_WIDTH(11);
