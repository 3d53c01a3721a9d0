// Two-dimensional SumThreshold flagger (reference rfi/twodflag.py:236-482), one batch of
// baselines per ksp_twodflag call.
//
// Every temporary is baseline-major, [baseline][time][averaged channel], as the
// reference's. The reference is sequential along every line it sums (box filter,
// cumulative sums, interpolation), so a lane here owns one line and runs the reference's
// loop in its order and precision; the parallelism is baselines x lines. Per-lane
// scratch lines are interleaved ([position][lane]) so that a wavefront's accesses to
// position i are contiguous. Medians are exact selections: per lane by a bitwise search
// on the order-preserving key of the float32 values, per (baseline, chunk) of the 2-D
// background by a workgroup radix select on LDS histograms (the pattern of madnz_long.h).
//
// Stages and kernels:
//   1 tdf_average          |z|, NaN / flags -> weight 0, frequency averaging
//   2 tdf_time_median      median spectrum over unflagged times
//     background (spectrum as a 1 x channels image, then the 2-D image):
//       tdf_init_work      working flags (and flags |= spectrum flags)
//       tdf_box_time       masked weight and data, box filter along time (or copy)
//       tdf_box_freq       box filter along frequency, in place
//       tdf_bg_reject      per chunk: median |residual| of unflagged, re-flag
//       tdf_interp_sub     background = data / weight, NaNs interpolated, data -= it
//   3/4 tdf_sum_threshold  SumThreshold per line and chunk (spectrum, time, frequency)
//   5 tdf_combine          spectrum | time | frequency flags, smeared in time
//   6 tdf_unavg_rows       replicated to the input channels, smeared, whole-row flags
//     tdf_unavg_cols       whole-channel flags
//   7 tdf_output           (time, freq, baseline) out = flags | isnan(data)
#include <cmath>

#include "hist_count.h"
#include "launch.h"

#define TDF_THREADS 256

namespace {

struct TdfWindows {
    int n;
    int w[KSP_TDF_MAX_WINDOWS];
    double tf[KSP_TDF_MAX_WINDOWS];
};

struct TdfChunks {
    int n;
    int ends[KSP_TDF_MAX_CHUNKS + 1];
};

__device__ __forceinline__ size_t tdf_gid() { return blockIdx.x * (size_t)blockDim.x + threadIdx.x; }

// float32 order as unsigned order (NaN patterns sort past the infinities)
__device__ __forceinline__ unsigned tdf_key(float x)
{
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tdf_unkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The k-th smallest key (0-based) of the valid elements: get(i, key) -> valid.
template <class G>
__device__ unsigned tdf_select(const G &get, int n, unsigned k)
{
    unsigned r = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = r | (1u << bit);
        unsigned cnt = 0;
        for (int i = 0; i < n; ++i) {
            unsigned key;
            if (get(i, key) && key < cand) ++cnt;
        }
        if (cnt <= k) r = cand;
    }
    return r;
}

// numba's np.median of `count` valid values (count >= 1): the middle value, or for an
// even count float32 (a + b) halved in float64 (arraymath.py _median_inner).
template <class G>
__device__ double tdf_median(const G &get, int n, int count)
{
    const unsigned half = (unsigned)count / 2;
    const unsigned hi = tdf_select(get, n, half);
    if (count & 1) return (double)tdf_unkey(hi);
    unsigned less = 0, below = 0;
    for (int i = 0; i < n; ++i) {
        unsigned key;
        if (get(i, key) && key < hi) {
            ++less;
            below = max(below, key);
        }
    }
    const unsigned lo = less >= half ? below : hi;
    const float sum = tdf_unkey(lo) + tdf_unkey(hi);
    return (double)sum / 2.0;
}

// ---------------------------------------------------------------- stage 1
template <bool AMP>
__global__ __launch_bounds__(TDF_THREADS) void tdf_average(
    const void *in, const uint8_t *in_flags, float *avg, uint8_t *flg, int T, int F, int A,
    int factor, int nb, int bl0, size_t stride_t, size_t stride_f)
{
    const size_t gid = tdf_gid();
    if (gid >= (size_t)T * A * nb) return;
    const int b = (int)(gid % nb);
    const size_t rest = gid / nb;
    const int fo = (int)(rest % A), t = (int)(rest / A);
    const int j0 = fo * factor, j1 = min(j0 + factor, F);
    float sum = 0.0f;
    int w = 0;
    for (int j = j0; j < j1; ++j) {
        const size_t idx = t * stride_t + j * stride_f + bl0 + b;
        float a;
        if (AMP) {
            a = fabsf(((const float *)in)[idx]);
        } else {
            const float2 z = ((const float2 *)in)[idx];
            a = ksp_abs_c64(z.x, z.y);
        }
        if (!in_flags[idx] && !isnan(a)) {
            sum += a;
            ++w;
        }
    }
    const size_t o = ((size_t)b * T + t) * A + fo;
    avg[o] = w == 0 ? 0.0f : __fdiv_rn(sum, (float)w);
    flg[o] = w == 0;
}

// ---------------------------------------------------------------- stage 2
__global__ __launch_bounds__(TDF_THREADS) void tdf_time_median(
    const float *avg, const uint8_t *flg, float *spec, uint8_t *spec_flg, int T, int A, int nb)
{
    const size_t lane = tdf_gid();
    if (lane >= (size_t)nb * A) return;
    const int b = (int)(lane / A), f = (int)(lane % A);
    const float *x = avg + (size_t)b * T * A + f;
    const uint8_t *fl = flg + (size_t)b * T * A + f;
    auto get = [&](int t, unsigned &key) {
        if (fl[(size_t)t * A]) return false;
        key = tdf_key(x[(size_t)t * A]);
        return true;
    };
    int count = 0;
    for (int t = 0; t < T; ++t) count += !fl[(size_t)t * A];
    if (count == 0) {
        spec[lane] = 0.0f;
        spec_flg[lane] = 1;
    } else {
        spec[lane] = (float)tdf_median(get, T, count);
        spec_flg[lane] = 0;
    }
}

// ---------------------------------------------------------------- background
// work = flags | extra[baseline][channel]; with `extra`, flags is updated as well
// (reference: flags |= spec_flags, twodflag.py:453).
__global__ __launch_bounds__(TDF_THREADS) void tdf_init_work(
    uint8_t *flags, const uint8_t *extra, uint8_t *work, int T, int A, int nb)
{
    const size_t gid = tdf_gid();
    if (gid >= (size_t)nb * T * A) return;
    uint8_t f = flags[gid] != 0;
    if (extra) {
        const size_t b = gid / ((size_t)T * A);
        f |= extra[b * A + gid % A];
        flags[gid] = f;
    }
    work[gid] = f;
}

// The four box passes of _box_gaussian_filter1d (twodflag.py:295-324) on one padded line
// P(0 .. n + 4r), sums in float64, in the reference's order.
template <class Acc>
__device__ void tdf_box_passes(const Acc &P, int n, int r)
{
    const int padding = 4 * r, L = n + padding, r2 = 2 * r;
    int prev_start = padding;
    for (int p = 1; p <= 4; ++p) {
        double s = 0.0;
        int start = padding - r2 * p;
        int stop = start + n + 2 * padding;
        start = max(start, 0);
        stop = min(stop, L);
        const int tail = min(stop, L - r2);
        for (int i = prev_start; i < min(start + r2, L); ++i) s += (double)P(i);
        for (int i = start; i < tail; ++i) {
            s += (double)P(i + r2);
            const float prev = P(i);
            P(i) = (float)s;
            s -= (double)prev;
        }
        for (int i = tail; i < stop; ++i) {
            const float prev = P(i);
            P(i) = (float)s;
            s -= (double)prev;
        }
        prev_start = start;
    }
}

// Lanes: (array, baseline, channel), array 0 = weight (not flagged), 1 = masked data.
// r == 0: no filtering along time, the masked arrays are written as they are.
__global__ __launch_bounds__(TDF_THREADS) void tdf_box_time(
    const float *data, const uint8_t *work, float *W, float *O, float *pad, int T, int A, int nb,
    size_t img, int r, float div)
{
    const size_t nl = 2 * (size_t)nb * A;
    const size_t lane = tdf_gid();
    if (lane >= nl) return;
    const int arr = (int)(lane / ((size_t)nb * A));
    const size_t rem = lane % ((size_t)nb * A);
    const size_t base = (rem / A) * img + rem % A;
    float *out = arr ? O : W;
    auto value = [&](int t) {
        const size_t i = base + (size_t)t * A;
        return work[i] ? 0.0f : (arr ? data[i] : 1.0f);
    };
    if (r == 0) {
        for (int t = 0; t < T; ++t) out[base + (size_t)t * A] = value(t);
        return;
    }
    auto P = [&](int i) -> float & { return pad[(size_t)i * nl + lane]; };
    const int padding = 4 * r;
    for (int i = 0; i < padding; ++i) P(i) = 0.0f;
    for (int t = 0; t < T; ++t) P(padding + t) = value(t);
    tdf_box_passes(P, T, r);
    for (int t = 0; t < T; ++t) out[base + (size_t)t * A] = __fdiv_rn(P(t), div);
}

// Lanes: (array, baseline, time); filters rows of W / O along frequency in place.
__global__ __launch_bounds__(TDF_THREADS) void tdf_box_freq(
    float *W, float *O, float *pad, int T, int A, int nb, size_t img, int r, float div)
{
    const size_t nl = 2 * (size_t)nb * T;
    const size_t lane = tdf_gid();
    if (lane >= nl) return;
    const int arr = (int)(lane / ((size_t)nb * T));
    const size_t rem = lane % ((size_t)nb * T);
    float *row = (arr ? O : W) + (rem / T) * img + (rem % T) * (size_t)A;
    auto P = [&](int i) -> float & { return pad[(size_t)i * nl + lane]; };
    const int padding = 4 * r;
    for (int i = 0; i < padding; ++i) P(i) = 0.0f;
    for (int f = 0; f < A; ++f) P(padding + f) = row[f];
    tdf_box_passes(P, A, r);
    for (int f = 0; f < A; ++f) row[f] = __fdiv_rn(P(f), div);
}

// masked_gaussian_filter's result (twodflag.py:390-400)
__device__ __forceinline__ float tdf_bg(const float *W, const float *O, size_t i)
{
    const float w = W[i];
    return w == 0.0f ? __builtin_nanf("") : __fdiv_rn(O[i], w);
}

// One workgroup per (baseline, chunk): threshold = median |data - background| of the
// unflagged samples (numba: float64) * reject_scale; samples above it are flagged
// (twodflag.py:44-59). Radix select on the 31-bit magnitude patterns, 8 bits a pass.
struct TdfSelectShared {
    unsigned hist[256];
    unsigned count;
    unsigned bin, below;
};

template <class G>
__device__ unsigned tdf_block_select(const G &get, size_t n, unsigned k, TdfSelectShared &sh)
{
    unsigned prefix = 0;
    for (int d = 3; d >= 0; --d) {
        const int shift = 8 * d;
        const unsigned hm = d == 3 ? 0u : ~((1u << (shift + 8)) - 1u);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) sh.hist[i] = 0;
        __syncthreads();
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
            unsigned key = 0;
            const bool hit = get(i, key) && (key & hm) == (prefix & hm);
            ksp_hist_count(sh.hist, (key >> shift) & 255u, hit);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned acc = 0, bin = 0;
            for (; bin < 255; ++bin) {
                if (acc + sh.hist[bin] > k) break;
                acc += sh.hist[bin];
            }
            sh.bin = bin;
            sh.below = acc;
        }
        __syncthreads();
        prefix |= sh.bin << shift;
        k -= sh.below;
        __syncthreads();
    }
    return prefix;
}

__global__ __launch_bounds__(TDF_THREADS) void tdf_bg_reject(
    const float *data, const float *W, const float *O, uint8_t *work, int T, int A, size_t img,
    TdfChunks ch, double reject_scale)
{
    __shared__ TdfSelectShared sh;
    const int c = blockIdx.x % ch.n;
    const size_t b = blockIdx.x / ch.n;
    const int c0 = ch.ends[c], width = ch.ends[c + 1] - c0;
    if (width <= 0) return;
    const size_t n = (size_t)T * width;
    auto index = [&](size_t i) { return b * img + (i / width) * A + c0 + i % width; };
    auto get = [&](size_t i, unsigned &key) {
        const size_t j = index(i);
        if (work[j]) return false;
        key = __float_as_uint(fabsf(data[j] - tdf_bg(W, O, j))) & 0x7fffffffu;
        return true;
    };
    if (threadIdx.x == 0) sh.count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) mine += !work[index(i)];
    atomicAdd(&sh.count, mine);
    __syncthreads();
    const unsigned count = sh.count;
    if (count == 0) return;  // NaN threshold: nothing is re-flagged
    const unsigned hi = tdf_block_select(get, n, count / 2, sh);
    double med;
    if (count & 1) {
        med = (double)__uint_as_float(hi);
    } else {
        const unsigned lo = tdf_block_select(get, n, count / 2 - 1, sh);
        const float sum = __uint_as_float(lo) + __uint_as_float(hi);
        med = (double)sum / 2.0;
    }
    const double thr = med * reject_scale;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
        const size_t j = index(i);
        const float res = fabsf(data[j] - tdf_bg(W, O, j));
        if ((double)res > thr) work[j] = 1;
    }
}

// Lanes: (baseline, time). Background row from W / O, NaNs linearly interpolated along
// frequency (_linearly_interpolate_nans1d, gradient and values in float64 as numba types
// them), then data -= background.
__global__ __launch_bounds__(TDF_THREADS) void tdf_interp_sub(
    float *data, const float *W, float *O, int T, int A, int nb, size_t img)
{
    const size_t lane = tdf_gid();
    if (lane >= (size_t)nb * T) return;
    const size_t base = (lane / T) * img + (lane % T) * (size_t)A;
    float *bg = O + base;
    for (int f = 0; f < A; ++f) bg[f] = tdf_bg(W, O, base + f);
    const int n = A;
    int p = 0;
    while (p < n && isnan(bg[p])) ++p;
    if (p == n) {
        for (int f = 0; f < n; ++f) bg[f] = 0.0f;
    } else {
        for (int f = 0; f < p; ++f) bg[f] = bg[p];
        ++p;
        while (p < n) {
            if (isnan(bg[p])) {
                int q = p + 1;
                while (q < n && isnan(bg[q])) ++q;
                if (q == n) {
                    for (int f = p; f < n; ++f) bg[f] = bg[p - 1];
                } else {
                    const float start = bg[p - 1];
                    const double grad = (double)(bg[q] - start) / (double)(q - (p - 1));
                    for (int f = p; f < q; ++f)
                        bg[f] = (float)((double)start + (double)(f - (p - 1)) * grad);
                }
                p = q;
            } else {
                ++p;
            }
        }
    }
    float *x = data + base;
    for (int f = 0; f < A; ++f) x[f] = x[f] - bg[f];
}

// ---------------------------------------------------------------- stages 3/4
// _sum_threshold1d (twodflag.py:94-161) for one line and chunk. along_time: lanes
// (baseline, channel), one chunk over all times; else lanes (baseline, time, chunk)
// along frequency with a halo of max(windows) - 1. Flags read are fa | fb.
__global__ __launch_bounds__(TDF_THREADS) void tdf_sum_threshold(
    const float *x, const uint8_t *fa, const uint8_t *fb, uint8_t *out, int T, int A, int nb,
    size_t img, int along_time, TdfWindows win, TdfChunks ch, double threshold_scale,
    double *cum, uint8_t *state)
{
    const size_t nl = along_time ? (size_t)nb * A : (size_t)nb * T * ch.n;
    const size_t lane = tdf_gid();
    if (lane >= nl) return;
    size_t base, stride;
    int n, c0, c1, p0, p1;
    if (along_time) {
        base = (lane / A) * img + lane % A;
        stride = A;
        n = T;
        c0 = p0 = 0;
        c1 = p1 = T;
    } else {
        const int c = (int)(lane % ch.n);
        const size_t rest = lane / ch.n;
        base = (rest / T) * img + (rest % T) * (size_t)A;
        stride = 1;
        n = A;
        c0 = ch.ends[c];
        c1 = ch.ends[c + 1];
        int maxw = win.w[0];
        for (int k = 1; k < win.n; ++k) maxw = max(maxw, win.w[k]);
        p0 = max(c0 - maxw + 1, 0);
        p1 = min(c1 + maxw - 1, n);
    }
    if (c1 <= c0) return;
    auto flagged = [&](int i) {
        const size_t j = base + (size_t)i * stride;
        return fa[j] || (fb && fb[j]);
    };
    auto X = [&](int i) { return x[base + (size_t)i * stride]; };
    // threshold: median |x| of the chunk's unflagged samples (float32), NaN -> inf
    auto get = [&](int i, unsigned &key) {
        if (flagged(c0 + i)) return false;
        key = tdf_key(fabsf(X(c0 + i)));
        return true;
    };
    int count = 0;
    for (int i = c0; i < c1; ++i) count += !flagged(i);
    float thr;
    if (count == 0) {
        thr = __builtin_inff();
    } else {
        const float med = (float)tdf_median(get, c1 - c0, count);
        thr = (float)((double)med * threshold_scale);
    }
    const int P = p1 - p0;
    auto C = [&](int i) -> double & { return cum[(size_t)i * nl + lane]; };
    auto S = [&](int i) -> uint8_t & { return state[(size_t)i * nl + lane]; };
    for (int i = 0; i < P; ++i) S(i) = 0;  // bit 0: positive, bit 1: negative
    for (int k = 0; k < win.n; ++k) {
        const int w = win.w[k];
        const double lim = (double)thr / win.tf[k];
        C(0) = 0.0;
        for (int i = 0; i < P; ++i) {
            double v = (double)X(p0 + i);
            const uint8_t s = S(i);
            if ((s & 1) && v > lim)
                v = lim;
            else if ((s & 2) && v < -lim)
                v = -lim;
            C(i + 1) = C(i) + v;
        }
        // _convolve_flags: a position is flagged when a window average starting in
        // [i - w + 1, i] is above the threshold
        const int m = P - w + 1;
        const float scale = (float)(1.0 / w);
        int last_pos = -0x3fffffff, last_neg = -0x3fffffff;
        for (int i = 0; i < P; ++i) {
            if (i < m) {
                const double avg = C(i + w) - C(i);
                if (avg * (double)scale > lim) last_pos = i;
                if (avg * (double)(-scale) > lim) last_neg = i;
            }
            uint8_t s = S(i);
            if (last_pos >= i - w + 1) s |= 1;
            if (last_neg >= i - w + 1) s |= 2;
            S(i) = s;
        }
    }
    for (int i = c0; i < c1; ++i) out[base + (size_t)i * stride] = S(i - p0) != 0;
}

// ---------------------------------------------------------------- stage 5
// Lanes: (baseline, channel). _combine_flags (twodflag.py:292-323).
__global__ __launch_bounds__(TDF_THREADS) void tdf_combine(
    const uint8_t *spec_st, const uint8_t *tfl, const uint8_t *ffl, uint8_t *out, int T, int A,
    int nb, int time_extend)
{
    const size_t lane = tdf_gid();
    if (lane >= (size_t)nb * A) return;
    const size_t base = (lane / A) * (size_t)T * A + lane % A;
    const bool spec = spec_st[lane];
    auto flag = [&](int t) {
        const size_t j = base + (size_t)t * A;
        return (int)(spec || tfl[j] || ffl[j]);
    };
    const int lo = -(time_extend / 2), hi = lo + time_extend;
    int a = 0, e = 0, cnt = 0;
    for (int t = 0; t < T; ++t) {
        const int t0 = max(t + lo, 0), t1 = min(t + hi, T);
        for (; e < t1; ++e) cnt += flag(e);
        for (; a < t0; ++a) cnt -= flag(a);
        out[base + (size_t)t * A] = cnt != 0;
    }
}

// ---------------------------------------------------------------- stage 6
// Lanes: (baseline, time). _unaverage_freq's row part (twodflag.py:337-358).
__global__ __launch_bounds__(TDF_THREADS) void tdf_unavg_rows(
    const uint8_t *cfl, uint8_t *rowfl, uint8_t *rowall, int T, int A, int F, int nb,
    int factor, int freq_extend, double frac_freq)
{
    const size_t lane = tdf_gid();
    if (lane >= (size_t)nb * T) return;
    const uint8_t *in = cfl + lane * A;  // lane = b * T + t
    uint8_t *out = rowfl + lane * F;
    auto rep = [&](int f) { return (int)in[f / factor]; };
    const int lo = -(freq_extend / 2), hi = lo + freq_extend;
    int a = 0, e = 0, cnt = 0, tot = 0;
    for (int f = 0; f < F; ++f) {
        const int f0 = max(f + lo, 0), f1 = min(f + hi, F);
        for (; e < f1; ++e) cnt += rep(e);
        for (; a < f0; ++a) cnt -= rep(a);
        const int flag = cnt != 0;
        out[f] = flag;
        tot += flag;
    }
    rowall[lane] = (double)tot > frac_freq * (double)F;
}

// Lanes: (baseline, input channel). Whole-channel flags (twodflag.py:363-365), counted
// before the whole-row flags are applied, as the reference does.
__global__ __launch_bounds__(TDF_THREADS) void tdf_unavg_cols(
    const uint8_t *rowfl, uint8_t *colall, int T, int F, int nb, double frac_time)
{
    const size_t lane = tdf_gid();
    if (lane >= (size_t)nb * F) return;
    const size_t b = lane / F, f = lane % F;
    int cnt = 0;
    for (int t = 0; t < T; ++t) cnt += rowfl[(b * T + t) * F + f];
    colall[lane] = (double)cnt > (double)T * frac_time;
}

// ---------------------------------------------------------------- stage 7
template <bool AMP>
__global__ __launch_bounds__(TDF_THREADS) void tdf_output(
    const void *in, const uint8_t *rowfl, const uint8_t *rowall, const uint8_t *colall,
    uint8_t *out, int T, int F, int nb, int bl0, size_t stride_t, size_t stride_f)
{
    const size_t gid = tdf_gid();
    if (gid >= (size_t)T * F * nb) return;
    const int b = (int)(gid % nb);
    const size_t rest = gid / nb;
    const int f = (int)(rest % F), t = (int)(rest / F);
    const size_t idx = t * stride_t + f * stride_f + bl0 + b;
    bool nan;
    if (AMP) {
        nan = isnan(((const float *)in)[idx]);
    } else {
        const float2 z = ((const float2 *)in)[idx];
        nan = isnan(z.x) || isnan(z.y);
    }
    out[idx] = nan || rowfl[((size_t)b * T + t) * F + f] || rowall[(size_t)b * T + t] ||
               colall[(size_t)b * F + f];
}

// ---------------------------------------------------------------- host side
// Radius of the box filter for sigma (twodflag.py:355, passes = 4) and the float32
// divisor d ** 4, which numba computes in float32 by squaring (int_power_impl).
int tdf_radius(double sigma) { return (int)(0.5 * sqrt(12.0 * (sigma * sigma) / 4 + 1)); }
float tdf_divisor(int r)
{
    float a = (float)(2 * r + 1);
    a = a * a;
    return a * a;
}

struct TdfLayout {
    size_t avg, W, O, flg, work, tfl, ffl;
    size_t spec, specW, specO, specflg, specwork, specst;
    size_t rowfl, rowall, colall;
    size_t cum, state;
    size_t total;
    int r_time_max, r_freq_max, max_p;
};

size_t tdf_align(size_t x) { return (x + 255) & ~(size_t)255; }

int tdf_check(const ksp_twodflag_params *p)
{
    KSP_REQUIRE(p != nullptr, "NULL params");
    KSP_REQUIRE(p->n_time >= 1 && p->n_time <= KSP_TDF_MAX_TIME, "n_time outside 1..4096");
    KSP_REQUIRE(p->n_freq >= 1 && p->n_freq <= KSP_TDF_MAX_FREQ, "n_freq outside 1..65536");
    KSP_REQUIRE(p->average_freq >= 1 && p->average_freq <= (1 << 20), "average_freq outside 1..2^20");
    KSP_REQUIRE(p->n_windows_time >= 1 && p->n_windows_time <= KSP_TDF_MAX_WINDOWS,
                "n_windows_time outside 1..32");
    KSP_REQUIRE(p->n_windows_freq >= 1 && p->n_windows_freq <= KSP_TDF_MAX_WINDOWS,
                "n_windows_freq outside 1..32");
    for (int k = 0; k < p->n_windows_time; ++k) {
        KSP_REQUIRE(p->windows_time[k] >= 1 && p->windows_time[k] <= (1 << 20), "windows_time outside 1..2^20");
        KSP_REQUIRE(p->tf_time[k] > 0 && std::isfinite(p->tf_time[k]), "tf_time not positive");
    }
    const int A = (p->n_freq + p->average_freq - 1) / p->average_freq;
    for (int k = 0; k < p->n_windows_freq; ++k) {
        KSP_REQUIRE(p->windows_freq[k] >= 1 && p->windows_freq[k] <= A, "windows_freq outside 1..averaged channels");
        KSP_REQUIRE(p->tf_freq[k] > 0 && std::isfinite(p->tf_freq[k]), "tf_freq not positive");
    }
    KSP_REQUIRE(p->n_chunks >= 1 && p->n_chunks <= KSP_TDF_MAX_CHUNKS, "n_chunks outside 1..512");
    KSP_REQUIRE(p->chunk_ends[0] == 0 && p->chunk_ends[p->n_chunks] == A,
                "chunk_ends must run from 0 to the averaged channels");
    for (int c = 0; c < p->n_chunks; ++c)
        KSP_REQUIRE(p->chunk_ends[c] <= p->chunk_ends[c + 1], "chunk_ends decreasing");
    KSP_REQUIRE(p->background_iterations >= 0 && p->background_iterations <= 64,
                "background_iterations outside 0..64");
    KSP_REQUIRE(p->time_extend >= 0 && p->time_extend <= (1 << 30), "time_extend outside 0..2^30");
    KSP_REQUIRE(p->freq_extend >= 0 && p->freq_extend <= (1 << 30), "freq_extend outside 0..2^30");
    KSP_REQUIRE(p->spike_width_time >= 0 && p->spike_width_freq >= 0, "negative spike width");
    const int it = max(p->background_iterations, 1);
    KSP_REQUIRE(p->spike_width_time * it < 4000 && p->spike_width_freq * it < 4000,
                "spike width x iterations gives a box radius beyond 2047");
    KSP_REQUIRE(tdf_radius(p->spike_width_time * it) <= KSP_TDF_MAX_RADIUS &&
                    tdf_radius(p->spike_width_freq * it) <= KSP_TDF_MAX_RADIUS,
                "box radius beyond 2047");
    KSP_REQUIRE(std::isfinite(p->threshold_scale) && std::isfinite(p->reject_scale) &&
                    std::isfinite(p->flag_all_time_frac) && std::isfinite(p->flag_all_freq_frac),
                "non-finite scale or fraction");
    KSP_REQUIRE(p->is_amplitude == 0 || p->is_amplitude == 1, "is_amplitude not 0/1");
    return 0;
}

TdfLayout tdf_layout(const ksp_twodflag_params *p, int nb)
{
    TdfLayout L;
    const size_t T = p->n_time, F = p->n_freq;
    const size_t A = (F + p->average_freq - 1) / p->average_freq;
    L.r_time_max = L.r_freq_max = 0;
    for (int ef = max(p->background_iterations, 1); ef >= 1; --ef) {
        L.r_time_max = max(L.r_time_max, tdf_radius(ef * p->spike_width_time));
        L.r_freq_max = max(L.r_freq_max, tdf_radius(ef * p->spike_width_freq));
    }
    int maxw = 0, maxwidth = 0;
    for (int k = 0; k < p->n_windows_freq; ++k) maxw = max(maxw, p->windows_freq[k]);
    for (int c = 0; c < p->n_chunks; ++c)
        maxwidth = max(maxwidth, p->chunk_ends[c + 1] - p->chunk_ends[c]);
    L.max_p = (int)min((size_t)maxwidth + 2 * (size_t)(maxw - 1), A);
    const size_t TA = T * A * nb;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = tdf_align(o + bytes);
        return at;
    };
    L.avg = take(TA * 4);
    L.W = take(TA * 4);
    L.O = take(TA * 4);
    L.flg = take(TA);
    L.work = take(TA);
    L.tfl = take(TA);
    L.ffl = take(TA);
    L.spec = take(A * nb * 4);
    L.specW = take(A * nb * 4);
    L.specO = take(A * nb * 4);
    L.specflg = take(A * nb);
    L.specwork = take(A * nb);
    L.specst = take(A * nb);
    L.rowfl = take(T * F * nb);
    L.rowall = take(T * nb);
    L.colall = take(F * nb);
    // per-lane lines: box filters (float, two arrays), SumThreshold (float64 sums and
    // flag state) along time and along frequency
    const size_t box_t = 2 * nb * A * (T + 4 * (size_t)L.r_time_max) * 4;
    const size_t box_f = 2 * nb * T * (A + 4 * (size_t)L.r_freq_max) * 4;
    const size_t lanes_t = nb * A, lanes_f = nb * T * (size_t)p->n_chunks;
    const size_t cum = max(lanes_t * (T + 1), lanes_f * ((size_t)L.max_p + 1)) * 8;
    const size_t state = max(lanes_t * T, lanes_f * (size_t)L.max_p);
    L.cum = take(max(max(box_t, box_f), cum));
    L.state = take(state);
    L.total = o;
    return L;
}

size_t tdf_blocks(size_t lanes) { return (lanes + TDF_THREADS - 1) / TDF_THREADS; }

#define TDF_LAUNCH(kernel, lanes, ...)                                                   \
    do {                                                                                 \
        if ((lanes) > 0)                                                                 \
            hipLaunchKernelGGL(kernel, dim3((unsigned)tdf_blocks(lanes)), dim3(TDF_THREADS), \
                               0, s, __VA_ARGS__);                                       \
    } while (0)

// _get_background2d (twodflag.py:405-64) on nb images of T x A at `data`, image stride
// `img`; `work` holds the working flags on entry. The background is subtracted from
// `data` on return.
void tdf_background(hipStream_t s, float *data, uint8_t *work, float *W, float *O, float *pad,
                    int T, int A, int nb, size_t img, const ksp_twodflag_params *p,
                    double sw_time, double sw_freq, const TdfChunks &ch)
{
    auto filter = [&](int ef) {
        const int rt = tdf_radius(ef * sw_time), rf = tdf_radius(ef * sw_freq);
        TDF_LAUNCH(tdf_box_time, 2 * (size_t)nb * A, data, work, W, O, pad, T, A, nb, img, rt,
                   tdf_divisor(rt));
        if (rf > 0)
            TDF_LAUNCH(tdf_box_freq, 2 * (size_t)nb * T, W, O, pad, T, A, nb, img, rf,
                       tdf_divisor(rf));
    };
    for (int ef = p->background_iterations; ef >= 1; --ef) {
        filter(ef);
        hipLaunchKernelGGL(tdf_bg_reject, dim3((unsigned)(nb * ch.n)), dim3(TDF_THREADS), 0, s,
                           data, W, O, work, T, A, img, ch, p->reject_scale);
    }
    filter(1);
    TDF_LAUNCH(tdf_interp_sub, (size_t)nb * T, data, W, O, T, A, nb, img);
}

}  // namespace

extern "C" int ksp_twodflag_workspace(const ksp_twodflag_params *params, int batch, size_t *bytes)
{
    KSP_REQUIRE(bytes != nullptr, "NULL bytes");
    if (int rc = tdf_check(params)) return rc;
    KSP_REQUIRE(batch >= 1, "batch < 1");
    *bytes = tdf_layout(params, batch).total;
    return 0;
}

extern "C" int ksp_twodflag_layout(const ksp_twodflag_params *params, int batch,
                                   ksp_twodflag_offsets *out)
{
    KSP_REQUIRE(out != nullptr, "NULL out");
    if (int rc = tdf_check(params)) return rc;
    KSP_REQUIRE(batch >= 1, "batch < 1");
    const TdfLayout L = tdf_layout(params, batch);
    // where ksp_twodflag leaves each stage (the buffers named in its body)
    out->spec_flags = L.specflg;
    out->spec_background = L.specO;
    out->spec_residual = L.spec;
    out->spec_st = L.specst;
    out->flags = L.flg;
    out->background = L.O;
    out->residual = L.avg;
    out->time_flags = L.tfl;
    out->freq_flags = L.ffl;
    out->combined = L.work;
    out->row_flags = L.rowfl;
    out->row_all = L.rowall;
    out->col_all = L.colall;
    return 0;
}

extern "C" int ksp_twodflag(int device, void *stream, const void *data, const uint8_t *in_flags,
                            uint8_t *out_flags, int n_bl, long long stride_t, long long stride_f,
                            int bl0, int batch, const ksp_twodflag_params *params,
                            void *workspace, size_t workspace_bytes)
{
    KSP_REQUIRE(data != nullptr && in_flags != nullptr && out_flags != nullptr &&
                    workspace != nullptr,
                "NULL buffer");
    if (int rc = tdf_check(params)) return rc;
    const ksp_twodflag_params *p = params;
    KSP_REQUIRE(n_bl >= 1 && batch >= 1 && bl0 >= 0 && (long long)bl0 + batch <= n_bl,
                "baselines [bl0, bl0 + batch) outside [0, n_bl)");
    KSP_REQUIRE(stride_f >= n_bl && stride_t >= stride_f * p->n_freq, "strides too small");
    const TdfLayout L = tdf_layout(p, batch);
    KSP_REQUIRE(workspace_bytes >= L.total, "workspace too small");
    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;

    const int T = p->n_time, F = p->n_freq, nb = batch, factor = p->average_freq;
    const int A = (F + factor - 1) / factor;
    const size_t img = (size_t)T * A;
    char *ws = (char *)workspace;
    float *avg = (float *)(ws + L.avg), *W = (float *)(ws + L.W), *O = (float *)(ws + L.O);
    uint8_t *flg = (uint8_t *)(ws + L.flg), *work = (uint8_t *)(ws + L.work);
    uint8_t *tfl = (uint8_t *)(ws + L.tfl), *ffl = (uint8_t *)(ws + L.ffl);
    float *spec = (float *)(ws + L.spec), *specW = (float *)(ws + L.specW);
    float *specO = (float *)(ws + L.specO);
    uint8_t *specflg = (uint8_t *)(ws + L.specflg), *specwork = (uint8_t *)(ws + L.specwork);
    uint8_t *specst = (uint8_t *)(ws + L.specst);
    uint8_t *rowfl = (uint8_t *)(ws + L.rowfl), *rowall = (uint8_t *)(ws + L.rowall);
    uint8_t *colall = (uint8_t *)(ws + L.colall);
    double *cum = (double *)(ws + L.cum);
    float *pad = (float *)(ws + L.cum);
    uint8_t *state = (uint8_t *)(ws + L.state);

    TdfChunks ch;
    ch.n = p->n_chunks;
    for (int c = 0; c <= ch.n; ++c) ch.ends[c] = p->chunk_ends[c];
    TdfWindows wt, wf;
    wt.n = p->n_windows_time;
    wf.n = p->n_windows_freq;
    for (int k = 0; k < KSP_TDF_MAX_WINDOWS; ++k) {
        wt.w[k] = k < wt.n ? p->windows_time[k] : 1;
        wt.tf[k] = k < wt.n ? p->tf_time[k] : 1.0;
        wf.w[k] = k < wf.n ? p->windows_freq[k] : 1;
        wf.tf[k] = k < wf.n ? p->tf_freq[k] : 1.0;
    }

    // 1: average
    ksp_dispatch_bool(p->is_amplitude != 0, [&](auto AMP) {
        TDF_LAUNCH(tdf_average<AMP()>, img * nb, data, in_flags, avg, flg, T, F, A, factor, nb,
                   bl0, (size_t)stride_t, (size_t)stride_f);
    });
    // 2: spectrum: time median, background, SumThreshold along frequency
    TDF_LAUNCH(tdf_time_median, (size_t)nb * A, avg, flg, spec, specflg, T, A, nb);
    TDF_LAUNCH(tdf_init_work, (size_t)nb * A, specflg, (const uint8_t *)nullptr, specwork, 1, A, nb);
    tdf_background(s, spec, specwork, specW, specO, pad, 1, A, nb, (size_t)A, p, 0.0,
                   p->spike_width_freq, ch);
    TDF_LAUNCH(tdf_sum_threshold, (size_t)nb * ch.n, spec, specflg, (const uint8_t *)nullptr,
               specst, 1, A, nb, (size_t)A, 0, wf, ch, p->threshold_scale, cum, state);
    // flags |= spectrum flags; 3: 2-D background
    TDF_LAUNCH(tdf_init_work, img * nb, flg, specst, work, T, A, nb);
    tdf_background(s, avg, work, W, O, pad, T, A, nb, img, p, p->spike_width_time,
                   p->spike_width_freq, ch);
    // 4: SumThreshold along time, then along frequency with the time flags
    TDF_LAUNCH(tdf_sum_threshold, (size_t)nb * A, avg, flg, (const uint8_t *)nullptr, tfl, T, A,
               nb, img, 1, wt, ch, p->threshold_scale, cum, state);
    TDF_LAUNCH(tdf_sum_threshold, (size_t)nb * T * ch.n, avg, flg, tfl, ffl, T, A, nb, img, 0, wf,
               ch, p->threshold_scale, cum, state);
    // 5, 6, 7
    TDF_LAUNCH(tdf_combine, (size_t)nb * A, specst, tfl, ffl, work, T, A, nb, p->time_extend);
    TDF_LAUNCH(tdf_unavg_rows, (size_t)nb * T, work, rowfl, rowall, T, A, F, nb, factor,
               p->freq_extend, p->flag_all_freq_frac);
    TDF_LAUNCH(tdf_unavg_cols, (size_t)nb * F, rowfl, colall, T, F, nb, p->flag_all_time_frac);
    ksp_dispatch_bool(p->is_amplitude != 0, [&](auto AMP) {
        TDF_LAUNCH(tdf_output<AMP()>, (size_t)T * F * nb, data, rowfl, rowall, colall, out_flags,
                   T, F, nb, bl0, (size_t)stride_t, (size_t)stride_f);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
