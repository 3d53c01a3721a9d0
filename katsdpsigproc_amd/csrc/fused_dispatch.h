// Every entry point of the fused flagger that one translation unit defines and another
// calls, declared once: flagger_fused.hip (the dispatcher) and each defining file include
// this, so a changed parameter list is a compile error.
#pragma once
#include "fused_common.h"

// All flags start at zero; the kernels only write the (rare) non-zero ones. Only the
// `baselines` bytes of each row are cleared: `flags` may be a column block of a wider array,
// whose bytes between the rows belong to someone else. Contiguous rows (every launch whose
// width is a multiple of the 128-byte row alignment, the benchmark's among them) take one
// linear fill, anything else a fill kernel (flagger_fused.hip).
hipError_t fused_zero_flags(const FusedParams &p, hipStream_t s);

// up to 4096 channels, lanes of 64 channels, one odd WIDTH in 3 .. 31 other than 13: each
// flagger_fused_w*.hip instantiates its widths (fused_width.h)
template <int WIDTH>
int ksp_fused_launch_width(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                           hipEvent_t ev1);

// more than 4096 channels (flagger_fused_long.hip; beyond 8192: flagger_fused_long3.hip)
int ksp_fused_long_supported(int channels, int width);
int ksp_fused_launch_long(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                          hipEvent_t ev1);
int ksp_fused_launch_long3(int device, hipStream_t s, const FusedParams &p, hipEvent_t ev0,
                           hipEvent_t ev1);

// 4096 channels, whole strips of 8 baselines (flagger_ring.hip)
bool ksp_ring_supported(const FusedParams &p, int width);
int ksp_ring_launch(int width, int device, hipStream_t s, const FusedParams &p, int n_cu,
                    hipEvent_t ev0, hipEvent_t ev1);
