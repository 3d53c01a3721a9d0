// Fused flagger for median windows of 3, 5, 7 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(3);
KSP_FUSED_INSTANTIATE_WIDTH(5);
KSP_FUSED_INSTANTIATE_WIDTH(7);
