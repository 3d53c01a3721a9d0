// Fused flagger for median windows of 15, 17 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(15);
KSP_FUSED_INSTANTIATE_WIDTH(17);
