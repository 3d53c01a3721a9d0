// Fused flagger for median windows of 19, 21 channels (see flagger_fused_kernel.h).
#include "fused_width.h"

KSP_FUSED_INSTANTIATE_WIDTH(19);
KSP_FUSED_INSTANTIATE_WIDTH(21);
