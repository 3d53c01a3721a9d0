// ksp_fused_launch_width (fused_dispatch.h) defined, for the flagger_fused_w*.hip files:
// each instantiates it for a few widths, so that the widths compile in parallel.
#pragma once
#include "flagger_fused_kernel.h"

template <int WIDTH>
int ksp_fused_launch_width(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                           hipEvent_t ev1)
{
    return launch_fused<64, WIDTH>(device, s, p, ev0, ev1);
}

#define KSP_FUSED_INSTANTIATE_WIDTH(W)                                                        \
    template int ksp_fused_launch_width<W>(int, hipStream_t, const FusedParams &, hipEvent_t, \
                                           hipEvent_t)
