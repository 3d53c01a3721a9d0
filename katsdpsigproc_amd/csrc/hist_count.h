// LDS histogram update shared by the radix-select kernels (madnz_long.h,
// percentile_long.h).
#pragma once
#include "ksp_common.h"

// hist[bin] += 1 for every lane with `hit`; one atomic per wavefront when all those
// lanes share the bin (a constant or heavily tied row would otherwise serialise 64 ways
// on one LDS bank).
__device__ __forceinline__ void ksp_hist_count(unsigned *hist, unsigned bin, bool hit)
{
    if (!hit) return;
    const unsigned first = __builtin_amdgcn_readfirstlane(bin);
    const unsigned long long active = __ballot(1);
    if (__ballot(bin == first) == active) {
        if (__lane_id() == __ffsll((unsigned long long)active) - 1)
            atomicAdd(&hist[first], (unsigned)__popcll(active));
    } else {
        atomicAdd(&hist[bin], 1u);
    }
}
