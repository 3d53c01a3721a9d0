// madnz_t for long rows (16385..262144 channels), included by noise.hip after
// KSP_MAD_NORMAL: one 1024-thread workgroup per baseline finds the median of the
// non-zero |x| by radix select on the 31-bit magnitude patterns instead of holding the
// row in registers.
//
// Three histogram passes resolve the pattern of the target rank 11 + 11 + 9 bits at a
// time: pass 1 counts bits 30..20 of every non-zero pattern, pass 2 bits 19..9 of the
// patterns in the selected top bin, pass 3 bits 8..0 of those sharing the selected 22-bit
// prefix. After each pass a workgroup prefix scan over the bins (DPP scan inside a
// wavefront, 16 wavefront totals through LDS) picks the bin that holds the rank.
// Zeros are left out of the histograms: the median of the non-zero values has rank
// (n_nz) / 2 among them, which is the rank shift of reference rank.mako:261-266 with the
// zeros removed. For an even count the value of rank - 1 is the same pattern when it
// occurs below the rank as well, else the largest non-zero pattern below the target:
// pass 3 keeps the largest one below the 22-bit prefix and the pass-3 bins below the
// selected one hold the rest. The rounding is madnz_t_kernel's: float32 (a + b) * 0.5,
// then 1.4826 in float64, rounded once; no non-zero value gives NaN.
//
// NaN input: a NaN deviation takes no part, exactly like a zero (the definition is
// |x| > 0, which a NaN fails). Pass 1 counts the patterns 1 .. 0x7f800000 (+inf) only, so
// the count and the rank are those of the values that do take part. NaN patterns lie above
// every such value: where passes 2 and 3 count some (the median is +inf), they fill bins
// behind the one that holds the rank and change nothing. A row of nothing but NaN and zeros
// gives NaN. (tests/test_gpu_nan_deviations.py pins this against rfi.host.NoiseEstMADHost.)
//
// Rows of up to MADL_STAGE_MAX channels are kept in LDS as patterns by pass 1 (144 KiB
// at most, one workgroup per CU), so HBM is read once. Longer rows are read from global
// memory in every pass; the second and third reads mostly hit L2 / the Infinity Cache.
// Histogram updates are LDS atomics, aggregated to one atomic per wavefront when every
// counted lane of the wavefront hits the same bin (a constant row, a zero-heavy row),
// which would otherwise serialise 64 ways on one bank.
#pragma once
#include "hist_count.h"

#define MADL_THREADS 1024
#define MADL_WAVES (MADL_THREADS / KSP_WAVE)
#define MADL_STAGE_MAX 36864  // channels staged in LDS (144 KiB of patterns)
#define MADL_MAX_CHANNELS 262144
#define MADL_NONE 0xffffffffu  // not a channel (|x| patterns have bit 31 clear)

struct MadlScratch {
    unsigned hist[2048];
    int wave_total[MADL_WAVES];
    int sel_bin, sel_below;
    unsigned max_below;  // largest non-zero pattern below the target (even counts)
};

__device__ __forceinline__ unsigned madl_pat(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// Patterns of channels c .. c + 3 (c % 4 == 0); MADL_NONE from `channels` on, which is
// never read.
__device__ __forceinline__ uint4 madl_load4(const float *row, int c, int channels, bool vec)
{
    uint4 q;
    if (vec && c + 4 <= channels) {
        q = *(const uint4 *)(row + c);
        q.x &= 0x7fffffffu;
        q.y &= 0x7fffffffu;
        q.z &= 0x7fffffffu;
        q.w &= 0x7fffffffu;
    } else {
        q.x = c < channels ? madl_pat(row[c]) : MADL_NONE;
        q.y = c + 1 < channels ? madl_pat(row[c + 1]) : MADL_NONE;
        q.z = c + 2 < channels ? madl_pat(row[c + 2]) : MADL_NONE;
        q.w = c + 3 < channels ? madl_pat(row[c + 3]) : MADL_NONE;
    }
    return q;
}

// One histogram pass. PASS 1: bins = bits 30..20 of every pattern that is neither 0 nor a NaN's (and, when
// STAGED, the patterns are stored to `stage`); PASS 2: bits 19..9 of those whose top 11
// bits are `prefix`; PASS 3: bits 8..0 of those whose top 22 bits are `prefix`, returning
// this thread's largest non-zero pattern below prefix << 9 (0 if none).
template <int PASS, bool STAGED>
__device__ __forceinline__ unsigned madl_pass(const float *row, unsigned *stage, unsigned *hist,
                                              int channels, bool vec, unsigned prefix)
{
    constexpr int MSHIFT = PASS == 1 ? 31 : PASS == 2 ? 20 : 9;
    constexpr int BSHIFT = PASS == 1 ? 20 : PASS == 2 ? 9 : 0;
    constexpr unsigned BMASK = PASS == 3 ? 0x1ffu : 0x7ffu;
    const unsigned lim = PASS == 3 ? prefix << 9 : 0u;
    unsigned best = 0;
    auto one = [&](unsigned p) {
        // PASS 1: 1 <= p <= 0x7f800000 leaves out zeros, NaN and MADL_NONE
        const bool counts = PASS == 1 ? p - 1u < 0x7f800000u : (p != 0 && (p >> MSHIFT) == prefix);
        ksp_hist_count(hist, (p >> BSHIFT) & BMASK, counts);
        if (PASS == 3) best = max(best, (p != 0 && p < lim) ? p : 0u);
    };
    auto quad = [&](uint4 q) {
        one(q.x);
        one(q.y);
        one(q.z);
        one(q.w);
    };
    const int t = threadIdx.x;
    if (PASS == 1 || !STAGED) {
        // 4 loads of 16 B in flight per thread before any is used
        for (int base = 0; base < channels; base += 16 * MADL_THREADS) {
            uint4 q[4];
#pragma unroll
            for (int j = 0; j < 4; j++)
                q[j] = madl_load4(row, base + j * 4 * MADL_THREADS + 4 * t, channels, vec);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = base + j * 4 * MADL_THREADS + 4 * t;
                if (STAGED && c < channels) *(uint4 *)(stage + c) = q[j];
                quad(q[j]);
            }
        }
    } else {
        for (int c = 4 * t; c < channels; c += 4 * MADL_THREADS) quad(*(const uint4 *)(stage + c));
    }
    return best;
}

// Exclusive prefix of this thread's bins [per * t, per * t + per) and the total of the
// first `nbins` bins (call after the pass's barrier).
__device__ __forceinline__ int madl_scan(MadlScratch &s, int nbins, int &pre)
{
    const int t = threadIdx.x, lane = t & (KSP_WAVE - 1), wave = t / KSP_WAVE;
    const int per = nbins / MADL_THREADS > 0 ? nbins / MADL_THREADS : 1;
    int mine = 0;
    for (int k = 0; k < per; k++)
        if (per * t + k < nbins) mine += (int)s.hist[per * t + k];
    const int incl = ksp_wave_scan_dpp(mine);
    if (lane == KSP_WAVE - 1) s.wave_total[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MADL_WAVES; w++) {
        const int x = s.wave_total[w];
        before += w < wave ? x : 0;
        total += x;
    }
    pre = before + incl - mine;
    return total;
}

// The bin holding rank r (0-based among the counted values) and the count below it.
__device__ __forceinline__ void madl_pick(MadlScratch &s, int nbins, int pre, int r, int &bin,
                                          int &below)
{
    const int t = threadIdx.x;
    const int per = nbins / MADL_THREADS > 0 ? nbins / MADL_THREADS : 1;
    for (int k = 0; k < per; k++) {
        const int b = per * t + k;
        if (b < nbins) {
            const int h = (int)s.hist[b];
            if (pre <= r && r < pre + h) {
                s.sel_bin = b;
                s.sel_below = pre;
            }
            pre += h;
        }
    }
    __syncthreads();
    bin = s.sel_bin;
    below = s.sel_below;
}

__device__ __forceinline__ unsigned madl_wave_max(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, 64));
    return v;
}

template <bool STAGED>
__global__ __launch_bounds__(MADL_THREADS) void madnz_t_long_kernel(const float *__restrict__ in,
                                                                    float *__restrict__ noise,
                                                                    int channels, int stride,
                                                                    int vec)
{
    __shared__ MadlScratch s;
    extern __shared__ __attribute__((aligned(16))) unsigned stage[];  // STAGED: the patterns
    const int t = threadIdx.x;
    const float *row = in + (size_t)blockIdx.x * stride;
    for (int i = t; i < 2048; i += MADL_THREADS) s.hist[i] = 0;
    if (t == 0) s.max_below = 0;
    __syncthreads();

    madl_pass<1, STAGED>(row, stage, s.hist, channels, vec, 0u);
    __syncthreads();
    int pre;
    const int n_nz = madl_scan(s, 2048, pre);
    if (n_nz == 0) {  // workgroup-uniform: numpy's median of nothing
        if (t == 0) noise[blockIdx.x] = __builtin_nanf("");
        return;
    }
    const int rank = n_nz / 2;
    int b1, below1;
    madl_pick(s, 2048, pre, rank, b1, below1);
    for (int i = t; i < 2048; i += MADL_THREADS) s.hist[i] = 0;
    __syncthreads();

    madl_pass<2, STAGED>(row, stage, s.hist, channels, vec, (unsigned)b1);
    __syncthreads();
    madl_scan(s, 2048, pre);
    int b2, below2;
    madl_pick(s, 2048, pre, rank - below1, b2, below2);
    if (t < 512) s.hist[t] = 0;
    __syncthreads();

    const unsigned prefix = ((unsigned)b1 << 11) | (unsigned)b2;
    unsigned best = madl_pass<3, STAGED>(row, stage, s.hist, channels, vec, prefix);
    best = madl_wave_max(best);
    if ((t & (KSP_WAVE - 1)) == 0 && best != 0) atomicMax(&s.max_below, best);
    __syncthreads();
    madl_scan(s, 512, pre);
    int b3, below3;
    madl_pick(s, 512, pre, rank - below1 - below2, b3, below3);

    const unsigned target = (prefix << 9) | (unsigned)b3;
    float result = __uint_as_float(target);
    if (!(n_nz & 1)) {  // workgroup-uniform
        float prev = result;  // rank - 1 holds the same value unless nothing else is below
        if (below1 + below2 + below3 == rank) {
            // the largest non-zero pattern below the target: below the 22-bit prefix
            // (pass 3's maximum) or in a lower pass-3 bin
            if (t < b3 && s.hist[t] != 0) atomicMax(&s.max_below, (prefix << 9) | (unsigned)t);
            __syncthreads();
            prev = __uint_as_float(s.max_below);
        }
        result = __fmul_rn(__fadd_rn(result, prev), 0.5f);
    }
    if (t == 0) noise[blockIdx.x] = (float)((double)result * KSP_MAD_NORMAL);
}
