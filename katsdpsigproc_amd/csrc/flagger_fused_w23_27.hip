// Fused flagger for median windows of 23, 25, 27 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(23);
KSP_FUSED_INSTANTIATE_WIDTH(25);
KSP_FUSED_INSTANTIATE_WIDTH(27);
