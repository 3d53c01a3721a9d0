// percentile5 for long rows (16385..65536 columns), included by percentile.hip after
// key_to_float: one 1024-thread workgroup per row holds the row in registers (VT <= 64
// values per thread, so HBM is read once) and finds the three ranks by radix select.
//
// Values become 32-bit keys that order like the floats (the transform of
// percentile5_wave_kernel), so signed input is exact. Min and max are reductions over the
// keys. The ranks (n-1)/4, 3(n-1)/4 and (n-1)/2 ("lower" element) are resolved
// 11 + 11 + 10 key bits at a time by three LDS histogram passes:
//   pass 1 counts bits 31..21 of every key in one histogram shared by the three ranks;
//   pass 2 counts bits 20..10 of the keys in each rank's selected top bin, one histogram
//          per rank (the ranks' prefixes can diverge);
//   pass 3 counts bits 9..0 of the keys sharing each rank's 22-bit prefix.
// After each pass a workgroup prefix scan (DPP scan inside a wavefront, 16 wavefront
// totals through LDS; the three histograms of a pass scanned together) picks each rank's
// bin. Histogram updates are LDS atomics, aggregated to one per wavefront when every
// counted lane of the wavefront hits the same bin (ksp_hist_count).
//
// Lane t holds columns PER * (g * 1024 + t) + [0, PER) for g = 0 .. VT / PER - 1, PER = 4
// float32 or 2 complex64 values: one 16-byte load each, 1 KiB contiguous per wavefront
// instruction, when the row allows 16-byte loads (vec_ok), else one element at a time.
// Columns beyond the range never count: their keys are 0 and are histogrammed like the
// others (no per-value test in the passes), and each bin 0 they reach -- in pass 1 always,
// in passes 2 and 3 when a rank's prefix is 0 -- is lowered by their number before the scan.
#pragma once
#include "hist_count.h"

#define P5L_THREADS 1024
#define P5L_WAVES (P5L_THREADS / KSP_WAVE)
#define P5L_MAX_COLUMNS (64 * P5L_THREADS)

struct P5lScratch {
    unsigned h1[2048];     // pass 1: key bits 31..21
    unsigned h2[3][2048];  // pass 2: key bits 20..10, per rank
    unsigned h3[3][1024];  // pass 3: key bits 9..0, per rank
    int wave_total[3][P5L_WAVES];
    int sel_bin[3], sel_below[3];
    unsigned kmin, kmax;
};

// Exclusive prefix, within each of NH histograms of NB bins (hist[h * NB + bin]), of this
// thread's bins [PER t, PER t + PER), PER = NB / 1024 (call after the pass's barrier).
template <int NH, int NB>
__device__ __forceinline__ void p5l_scan(P5lScratch &s, const unsigned *hist, int (&pre)[NH])
{
    constexpr int PER = NB / P5L_THREADS;
    const int t = threadIdx.x, lane = t & (KSP_WAVE - 1), wave = t / KSP_WAVE;
    int mine[NH], incl[NH];
#pragma unroll
    for (int h = 0; h < NH; h++) {
        mine[h] = 0;
#pragma unroll
        for (int k = 0; k < PER; k++) mine[h] += (int)hist[h * NB + PER * t + k];
        incl[h] = ksp_wave_scan_dpp(mine[h]);
        if (lane == KSP_WAVE - 1) s.wave_total[h][wave] = incl[h];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NH; h++) {
        int before = 0;
#pragma unroll
        for (int w = 0; w < P5L_WAVES; w++) before += w < wave ? s.wave_total[h][w] : 0;
        pre[h] = before + incl[h] - mine[h];
    }
}

// For each rank j: the bin of histogram `hist + (NH == 1 ? 0 : j) * NB` that holds rank
// r[j] (0-based among the keys counted there), and the count below that bin.
template <int NH, int NB>
__device__ __forceinline__ void p5l_pick(P5lScratch &s, const unsigned *hist, const int (&pre)[NH],
                                         const int (&r)[3], int (&bin)[3], int (&below)[3])
{
    constexpr int PER = NB / P5L_THREADS;
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int h = NH == 1 ? 0 : j;
        int p = pre[h];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int b = PER * t + k;
            const int c = (int)hist[h * NB + b];
            if (p <= r[j] && r[j] < p + c) {
                s.sel_bin[j] = b;
                s.sel_below[j] = p;
            }
            p += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; j++) {
        bin[j] = s.sel_bin[j];
        below[j] = s.sel_below[j];
    }
}

template <int VT, bool IS_AMP>
__global__ __launch_bounds__(P5L_THREADS) void percentile5_long_kernel(
    const void *__restrict__ in, float *__restrict__ out, int rows, int in_stride, int out_stride,
    int first_col, int n_cols, int vec_ok)
{
    constexpr int PER = IS_AMP ? 4 : 2;  // columns per 16-byte load
    static_assert(VT % 4 == 0 && VT <= 64, "VT: a multiple of 4, at most 64");
    __shared__ P5lScratch s;
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    for (int i = t; i < 2048; i += P5L_THREADS) s.h1[i] = 0;
    for (int i = t; i < 3 * 2048; i += P5L_THREADS) (&s.h2[0][0])[i] = 0;
    for (int i = t; i < 3 * 1024; i += P5L_THREADS) (&s.h3[0][0])[i] = 0;
    if (t == 0) {
        s.kmin = 0xffffffffu;
        s.kmax = 0;
    }

    // Every load is issued without a branch, so that they are all in flight together: a
    // lane whose group is not wholly in the range re-reads the row's first PER columns
    // (and its keys become 0); the one group that straddles the end of the range is read
    // afterwards, a column at a time.
    // (the row's address is uniform: 32-bit column offsets from it keep one VGPR per load)
    const float *rowf = (const float *)in + (IS_AMP ? 1 : 2) * ((size_t)row * in_stride + first_col);
    unsigned key[VT];
    unsigned kmin = 0xffffffffu, kmax = 0;
    auto to_key = [&](float a, bool ok) __attribute__((always_inline)) {
        const unsigned u = __float_as_uint(a);
        const unsigned k = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
        kmin = min(kmin, ok ? k : 0xffffffffu);
        kmax = max(kmax, ok ? k : 0u);
        return ok ? k : 0u;
    };
    auto load = [&](unsigned c) __attribute__((always_inline)) {
        if (IS_AMP) return rowf[c];
        const float2 z = ((const float2 *)rowf)[c];
        return ksp_abs_c64(z.x, z.y);
    };
    if (vec_ok) {
#pragma unroll
        for (int g = 0; g < VT / PER; g++) {
            const int c = PER * (g * P5L_THREADS + t);
            const bool full = c + PER <= n_cols;
            const unsigned cl = full ? c : 0;
            unsigned *k = key + PER * g;
            if (IS_AMP) {
                const float4 q = *(const float4 *)(rowf + cl);
                k[0] = to_key(q.x, full);
                k[1] = to_key(q.y, full);
                k[2] = to_key(q.z, full);
                k[3] = to_key(q.w, full);
            } else {
                const float4 q = *(const float4 *)((const float2 *)rowf + cl);
                k[0] = to_key(ksp_abs_c64(q.x, q.y), full);
                k[1] = to_key(ksp_abs_c64(q.z, q.w), full);
            }
        }
        const int c_tail = n_cols - n_cols % PER;  // first column of the straddling group
        if (c_tail < n_cols && (c_tail / PER) % P5L_THREADS == t) {
#pragma unroll
            for (int g = 0; g < VT / PER; g++) {
                if (PER * (g * P5L_THREADS + t) == c_tail) {
#pragma unroll
                    for (int p = 0; p < PER; p++) {
                        const bool ok = c_tail + p < n_cols;
                        key[PER * g + p] = to_key(load(ok ? c_tail + p : 0), ok);
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VT; j++) {
            const int c = PER * ((j / PER) * P5L_THREADS + t) + j % PER;
            const bool ok = c < n_cols;
            key[j] = to_key(load(ok ? c : 0), ok);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off, 64));
    }
    __syncthreads();  // histograms cleared
    if ((t & (KSP_WAVE - 1)) == 0) {
        atomicMin(&s.kmin, kmin);
        atomicMax(&s.kmax, kmax);
    }

    const unsigned n_pad = (unsigned)(VT * P5L_THREADS - n_cols);  // keys beyond the range
    const int r[3] = {(n_cols - 1) / 4, ((n_cols - 1) * 3) / 4, (n_cols - 1) / 2};
    int pre1[1], pre3[3], b1[3], below1[3], b2[3], below2[3], b3[3], below3[3];

    // pass 1: bits 31..21 of every key
#pragma unroll
    for (int j = 0; j < VT; j++) ksp_hist_count(s.h1, key[j] >> 21, true);
    if (t == 0) atomicSub(&s.h1[0], n_pad);
    __syncthreads();
    p5l_scan<1, 2048>(s, s.h1, pre1);
    p5l_pick<1, 2048>(s, s.h1, pre1, r, b1, below1);

    // pass 2: bits 20..10 of the keys in each rank's top bin
    // (the prefix tests are written as (key ^ prefix) < 2^k rather than key >> k == prefix:
    // a shift shared with the previous pass would keep VT more values live across it)
    int r2[3];
    unsigned top1[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        r2[q] = r[q] - below1[q];
        top1[q] = (unsigned)b1[q] << 21;
    }
#pragma unroll
    for (int j = 0; j < VT; j++) {
        const unsigned bin = (key[j] >> 10) & 0x7ffu;
#pragma unroll
        for (int q = 0; q < 3; q++) ksp_hist_count(s.h2[q], bin, (key[j] ^ top1[q]) < (1u << 21));
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (t == q && b1[q] == 0) atomicSub(&s.h2[q][0], n_pad);
    __syncthreads();
    p5l_scan<3, 2048>(s, &s.h2[0][0], pre3);
    p5l_pick<3, 2048>(s, &s.h2[0][0], pre3, r2, b2, below2);

    // pass 3: bits 9..0 of the keys sharing each rank's 22-bit prefix
    unsigned prefix[3];
    int r3[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        prefix[q] = ((unsigned)b1[q] << 11) | (unsigned)b2[q];
        r3[q] = r2[q] - below2[q];
    }
#pragma unroll
    for (int j = 0; j < VT; j++) {
        const unsigned bin = key[j] & 0x3ffu;
#pragma unroll
        for (int q = 0; q < 3; q++) ksp_hist_count(s.h3[q], bin, (key[j] ^ (prefix[q] << 10)) < (1u << 10));
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (t == q && prefix[q] == 0) atomicSub(&s.h3[q][0], n_pad);
    __syncthreads();
    p5l_scan<3, 1024>(s, &s.h3[0][0], pre3);
    p5l_pick<3, 1024>(s, &s.h3[0][0], pre3, r3, b3, below3);

    if (t == 0) {
        out[0 * (size_t)out_stride + row] = key_to_float(s.kmin);
        out[1 * (size_t)out_stride + row] = key_to_float(s.kmax);
        out[2 * (size_t)out_stride + row] = key_to_float((prefix[0] << 10) | (unsigned)b3[0]);
        out[3 * (size_t)out_stride + row] = key_to_float((prefix[1] << 10) | (unsigned)b3[1]);
        out[4 * (size_t)out_stride + row] = key_to_float((prefix[2] << 10) | (unsigned)b3[2]);
    }
}
