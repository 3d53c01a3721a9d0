// Fused flagger for 4097 .. 12288 channels (flagger_long_kernel.h): 4097 .. 8192 channels,
// two groups of runs per lane, are compiled here.
#include "flagger_long_kernel.h"

int ksp_fused_long_supported(int channels, int width)
{
    return width == 13 && channels > 4096 && channels <= 12288 && long_fits(channels, 3);
}

int ksp_fused_launch_long(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                          hipEvent_t ev1)
{
    if (p.channels <= 8192) return launch_long<2, 4, 13>(device, s, p, ev0, ev1);  // 4 x 8192 always fit
    return ksp_fused_launch_long3(device, s, p, ev0, ev1);
}
