// Fused flagger for 8193 .. 12288 channels (flagger_long_kernel.h): three groups of runs
// per lane, strips of 4 baselines while they fit in LDS, else of 3.
#include "flagger_long_kernel.h"

int ksp_fused_launch_long3(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                           hipEvent_t ev1)
{
    if (long_fits(p.channels, 4)) return launch_long<3, 4, 13>(device, s, p, ev0, ev1);
    return launch_long<3, 3, 13>(device, s, p, ev0, ev1);
}
