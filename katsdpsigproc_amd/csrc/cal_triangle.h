// The load phase of the solvers that keep a channel's matrix in LDS (solve_jones; solve_gains
// has the same walk written out in its kernel): the threads of a workgroup walk the upper
// triangle of `pairs`, gather the samples its entries name and fill the upper triangle of
// A = w v and W = w, 12 bytes per pair in three float arrays of n (n - 1) / 2 elements, element
// (p, q), p < q, at p (2 n - p - 1) / 2 + (q - p - 1). An entry is validated before anything is
// derived from it: 0, or one whose magnitude exceeds `baselines` (INT32_MIN included, compared
// without negating it), forms no address: its thread reads baseline 0 instead, which always
// exists, and drops it, so that a thread's loads need no branch and KSP_TRIANGLE_UNROLL
// elements are in flight at once (first their entries, then their samples). Device code only.
#pragma once
#include "cal_math.h"

#define KSP_TRIANGLE_UNROLL 8  // elements of the triangle a thread loads at once

// The flat index of element (lo, hi), lo < hi, of a triangle over n inputs
__device__ __forceinline__ int ksp_triangle_index(int n, int lo, int hi)
{
    return lo * (2 * n - lo - 1) / 2 + (hi - lo - 1);
}

// Fill a_re, a_im, a_w (LDS, n (n - 1) / 2 elements each) from one channel's rows of vis,
// weights and flags, and set has[p] = 1 for every input with a kept sample (the caller has
// zeroed `has` and passed a barrier; it passes another before it reads what is written here).
// A sample is kept when its entry is valid, neither part of v is NaN, w > 0 (1 without
// HAS_W) and (flags & mask) == 0; with SAME_ANTENNA_IS_NONE an entry whose inputs have
// p / 2 == q / 2 is no baseline either. Everything else stores +0.
template <bool HAS_W, bool HAS_F, bool SAME_ANTENNA_IS_NONE>
__device__ __forceinline__ void ksp_triangle_load(
    const float2 *__restrict__ vis_row, const float *__restrict__ weights_row,
    const uint8_t *__restrict__ flags_row, const int *__restrict__ pairs, long long pairs_stride,
    int baselines, int n, unsigned mask, float *a_re, float *a_im, float *a_w, int *has, int tid,
    int threads)
{
    const int n_pairs = n * (n - 1) / 2;
    int p = 0, row = 0;  // row: the flat index of (p, p + 1)
    for (int e0 = tid; e0 < n_pairs; e0 += KSP_TRIANGLE_UNROLL * threads) {
        int pp[KSP_TRIANGLE_UNROLL], qq[KSP_TRIANGLE_UNROLL], t[KSP_TRIANGLE_UNROLL];
#pragma unroll
        for (int u = 0; u < KSP_TRIANGLE_UNROLL; u++) {
            const int e = e0 + u * threads;
            pp[u] = -1;
            qq[u] = 0;
            if (e < n_pairs) {
                while (e >= row + (n - 1 - p)) {
                    row += n - 1 - p;
                    p++;
                }
                pp[u] = p;
                qq[u] = p + 1 + (e - row);
            }
        }
#pragma unroll
        for (int u = 0; u < KSP_TRIANGLE_UNROLL; u++)
            t[u] = pp[u] >= 0 ? pairs[pp[u] * pairs_stride + qq[u]] : 0;
        float2 v[KSP_TRIANGLE_UNROLL];
        float ws[KSP_TRIANGLE_UNROLL];
        unsigned f[KSP_TRIANGLE_UNROLL];
        bool valid[KSP_TRIANGLE_UNROLL];
#pragma unroll
        for (int u = 0; u < KSP_TRIANGLE_UNROLL; u++) {
            valid[u] = t[u] > 0 ? t[u] <= baselines : (t[u] < 0 && t[u] >= -baselines);
            if (SAME_ANTENNA_IS_NONE) valid[u] = valid[u] && (pp[u] >> 1) != (qq[u] >> 1);
            const long long at = valid[u] ? (t[u] > 0 ? t[u] : -t[u]) - 1 : 0;
            v[u] = vis_row[at];
            ws[u] = HAS_W ? weights_row[at] : 1.0f;
            f[u] = HAS_F ? flags_row[at] : 0u;
        }
#pragma unroll
        for (int u = 0; u < KSP_TRIANGLE_UNROLL; u++) {
            if (pp[u] < 0) continue;
            const bool kept = valid[u] && !__builtin_isnan(v[u].x) && !__builtin_isnan(v[u].y) &&
                              ws[u] > 0.0f && (f[u] & mask) == 0;
            float re = 0.0f, im = 0.0f, w = 0.0f;
            if (kept) {
                re = __fmul_rn(ws[u], v[u].x);
                im = __fmul_rn(ws[u], v[u].y);
                if (t[u] < 0) im = -im;
                w = ws[u];
                has[pp[u]] = 1;  // (every writer stores the same value)
                has[qq[u]] = 1;
            }
            const int e = e0 + u * threads;
            a_re[e] = re;
            a_im[e] = im;
            a_w[e] = w;
        }
    }
}
