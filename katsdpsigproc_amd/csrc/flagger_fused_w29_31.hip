// Fused flagger for median windows of 29, 31 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(29);
KSP_FUSED_INSTANTIATE_WIDTH(31);
