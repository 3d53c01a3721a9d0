// interpolate_gains: per input, the gains of ksp_solve_gains filled across the channels the
// solver left without a value, in one launch (no reference counterpart): the delay model of
// ksp_fit_delays divided out, a running mean over the kept channels, the mean amplitude
// normalised, gaps of up to max_gap channels interpolated linearly (held at the ends of the
// band), the model and a band-wide gain multiplied back in, and optionally the reciprocal.
// rfi/host.py InterpolateGainsHost is the definition; the kernel reproduces it bit for bit, so
// every step is one float32 operation, rounded once (the translation unit is built with
// -ffp-contract=off and correctly rounded division and square root, and the steps are written
// with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, which are never contracted; the one square
// root is __builtin_sqrtf, which that build flag expands to the correctly rounded sequence).
//
//   per input p:
//   kept[c]: both parts of g = gains[c][p] finite, status[c] & mask == 0, both parts of
//     m = model[c][p] finite;  n_kept counts them;  none: bit 0, the column is NaN
//   d = (g.re m.re + g.im m.im, g.im m.re - g.re m.im)                  (g without model)
//   s[c] = (sum of d over the kept channels of [c - smooth/2, c + smooth/2], ascending
//     from +0) / float(their number), per part, for a kept c            (d for smooth = 1)
//   a = (halving tree over Cpad terms of sqrt(s.re s.re + s.im s.im), +0 where not kept)
//     / float(n_kept);  a in (0, inf): s = (s.re / a, s.im / a), else bit 0, the column is NaN
//   for a c that is not kept, with l / r the nearest kept channel below / above:
//     both and r - l - 1 <= max_gap: t = float(c - l) / float(r - l),
//       y = s[l] + (s[r] - s[l]) t per part
//     only l and c - l <= max_gap: y = s[l];  only r and r - c <= max_gap: y = s[r]
//     otherwise y = NaN and bit 1;  y = s[c] for a kept c
//   y = (y.re m.re - y.im m.im, y.re m.im + y.im m.re), then the same with scale[p]
//   corrections: q = y.re y.re + y.im y.im;  y = q > 0 ? (y.re / q, -y.im / q) : NaN
//
// One workgroup per input; its column of d (then s) lies in `channels` complex64 of dynamic LDS
// (128 KiB at 16384). The workgroup has Cpad threads (the next power of two at or above
// channels), at least 64 and at most 1024; thread i owns channels i, i + T, i + 2 T, ...
// (at most IG_PER_THREAD = 16), so a wavefront's channels of one round are 64 adjacent ones.
// The columns are read and written with 8-byte accesses at a stride of *_stride elements: all
// workgroups touch the same lines, which therefore come from L2. The model stays in registers
// from the first read to the last multiplication.
//
// The ballot of `kept` over a wavefront is the 64-bit word of those 64 channels, and the words
// (at most 256) are the whole book-keeping. The first 256 threads scan them: the highest kept
// channel at or below the end of each word is an inclusive max-scan, the lowest at or above its
// start a reverse min-scan, and n_kept a sum of population counts, each by lane shuffles within
// a wavefront and through LDS across the (at most four) wavefronts. A channel then finds its
// neighbours in its own word by counting zeros, and in the scans of the words next to it
// otherwise. The window of the running mean reads the words and the column from LDS; the new
// values wait in registers for a barrier before they replace the old ones. The upper levels of
// the amplitude's tree are thread-local (terms i + m T of a thread pair up exactly as the tree
// pairs them), the next ones go through LDS, the last six through lane shuffles.
// Every decision about the column is taken from the same values by every thread: uniform over
// the workgroup. An input is read completely before the first store, so `out` may be `gains`.
// Row offsets are size_t. No atomics, no workspace, no dependence on the order of workgroups.
// Padding is neither read nor written.
#include "cal_math.h"
#include "launch.h"

#define IG_MAX_CHANNELS 16384
#define IG_MAX_GAP 16384
#define IG_MAX_SMOOTH 31
#define IG_MAX_THREADS 1024
#define IG_PER_THREAD (IG_MAX_CHANNELS / IG_MAX_THREADS)
#define IG_MAX_WORDS (IG_MAX_CHANNELS / 64)
#define IG_SCAN_WAVES (IG_MAX_WORDS / 64)
#define IG_NO_DATA 1
#define IG_GAP_LEFT 2
#define IG_NONE_ABOVE 0x7fffffff

typedef unsigned long long ig_word;

static int ig_threads(int c_pad)
{
    return c_pad < 64 ? 64 : c_pad > IG_MAX_THREADS ? IG_MAX_THREADS : c_pad;
}

__device__ __forceinline__ int ig_highest(ig_word word) { return 63 - __clzll((long long)word); }
__device__ __forceinline__ int ig_lowest(ig_word word) { return __ffsll(word) - 1; }

__global__ __launch_bounds__(IG_MAX_THREADS) void interpolate_gains_kernel(
    const float2 *gains, const uint8_t *__restrict__ status, const float2 *__restrict__ model,
    const float2 *__restrict__ scale, float2 *out, int *__restrict__ kept_out,
    int *__restrict__ filled_out, uint8_t *__restrict__ fill_status,
    float *__restrict__ mean_amplitude, int channels, size_t gains_stride, size_t model_stride,
    size_t out_stride, int c_pad, int per_thread, int max_gap, int smooth, unsigned mask,
    int corrections)
{
    extern __shared__ float2 ig_col[];
    __shared__ ig_word words[IG_MAX_WORDS];
    __shared__ int below[IG_MAX_WORDS], above[IG_MAX_WORDS];
    __shared__ int wave_lo[IG_SCAN_WAVES], wave_hi[IG_SCAN_WAVES], wave_kept[IG_SCAN_WAVES];
    __shared__ float partial[IG_MAX_THREADS / 2];
    __shared__ int wave_filled[IG_MAX_THREADS / 64], wave_gap[IG_MAX_THREADS / 64];
    __shared__ float shared_a;
    const int tid = threadIdx.x, threads = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int waves = threads >> 6;
    const size_t p = blockIdx.x;
    const float nan32 = __builtin_nanf("");

    // ---- load, de-rotate, and the words of `kept`
    float2 mm[IG_PER_THREAD];
#pragma unroll
    for (int m = 0; m < IG_PER_THREAD; m++) {
        mm[m] = make_float2(1.0f, 0.0f);
        if (m < per_thread) {
            const int c = tid + m * threads;
            bool keep = false;
            if (c < channels) {
                float2 d = gains[(size_t)c * gains_stride + p];
                keep = ksp_cfinite(d);
                if (status != nullptr) keep = keep && (status[c] & mask) == 0;
                if (model != nullptr) {
                    const float2 mc = model[(size_t)c * model_stride + p];
                    mm[m] = mc;
                    keep = keep && ksp_cfinite(mc);
                    d = ksp_cmul_conj(d, mc);
                }
                ig_col[c] = d;
            }
            const ig_word ballot = __ballot(keep);
            if (lane == 0) words[m * waves + wave] = ballot;
        }
    }
    __syncthreads();

    // ---- per word: the nearest kept channel at or below its end and at or above its start
    const int n_words = per_thread * waves;
    const int scan_waves = waves < IG_SCAN_WAVES ? waves : IG_SCAN_WAVES;
    int lo = -1, hi = IG_NONE_ABOVE;
    if (tid < IG_MAX_WORDS) {  // (whole wavefronts)
        const ig_word word = tid < n_words ? words[tid] : 0;
        int count = __popcll(word);
        if (word != 0) {
            lo = 64 * tid + ig_highest(word);
            hi = 64 * tid + ig_lowest(word);
        }
        for (int n = 1; n < 64; n *= 2) {
            const int other_lo = __shfl_up(lo, (unsigned)n);
            const int other_hi = __shfl_down(hi, (unsigned)n);
            if (lane >= n && other_lo > lo) lo = other_lo;
            if (lane + n < 64 && other_hi < hi) hi = other_hi;
            count += __shfl_xor(count, n);
        }
        if (lane == 63) wave_lo[wave] = lo;
        if (lane == 0) {
            wave_hi[wave] = hi;
            wave_kept[wave] = count;
        }
    }
    __syncthreads();
    if (tid < IG_MAX_WORDS) {
        for (int w = 0; w < wave; w++) lo = wave_lo[w] > lo ? wave_lo[w] : lo;
        for (int w = wave + 1; w < scan_waves; w++) hi = wave_hi[w] < hi ? wave_hi[w] : hi;
        below[tid] = lo;
        above[tid] = hi;
    }
    int n_kept = 0;
    for (int w = 0; w < scan_waves; w++) n_kept += wave_kept[w];
    __syncthreads();

    // ---- the running mean over the kept channels of the window
    if (smooth > 1) {
        const int reach = smooth >> 1;
        float2 mean[IG_PER_THREAD];
#pragma unroll
        for (int m = 0; m < IG_PER_THREAD; m++) {
            mean[m] = make_float2(0.0f, 0.0f);
            const int c = tid + m * threads;
            if (m < per_thread && c < channels && (words[c >> 6] >> (c & 63) & 1) != 0) {
                const int first = c - reach < 0 ? 0 : c - reach;
                const int last = c + reach > channels - 1 ? channels - 1 : c + reach;
                float re = 0.0f, im = 0.0f;
                int n = 0;
                for (int j = first; j <= last; j++)
                    if ((words[j >> 6] >> (j & 63) & 1) != 0) {
                        const float2 d = ig_col[j];
                        re = __fadd_rn(re, d.x);
                        im = __fadd_rn(im, d.y);
                        n++;
                    }
                mean[m] = make_float2(__fdiv_rn(re, (float)n), __fdiv_rn(im, (float)n));
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < IG_PER_THREAD; m++) {
            const int c = tid + m * threads;
            if (m < per_thread && c < channels && (words[c >> 6] >> (c & 63) & 1) != 0)
                ig_col[c] = mean[m];
        }
        __syncthreads();
    }

    // ---- the mean amplitude
    bool failed = n_kept == 0;
    if (mean_amplitude != nullptr) {
        float term[IG_PER_THREAD];
#pragma unroll
        for (int m = 0; m < IG_PER_THREAD; m++) {
            term[m] = 0.0f;
            const int c = tid + m * threads;
            if (m < per_thread && c < channels && (words[c >> 6] >> (c & 63) & 1) != 0) {
                const float2 s = ig_col[c];
                term[m] = __builtin_sqrtf(ksp_norm2(s));
            }
        }
        // the levels of the tree whose two terms belong to one thread: i + m T with i + (m + n) T
        const int local_terms = c_pad > threads ? c_pad / threads : 1;
#pragma unroll
        for (int n = IG_PER_THREAD / 2; n >= 1; n /= 2)
            if (n < local_terms) {
#pragma unroll
                for (int i = 0; i < n; i++) term[i] = __fadd_rn(term[i], term[i + n]);
            }
        float total = term[0];
        const int width = c_pad < threads ? c_pad : threads;
        // across wavefronts: the upper half hands its sums to the lower half
        for (int n = width / 2; n >= 64; n /= 2) {
            if (tid >= n && tid < 2 * n) partial[tid - n] = total;
            __syncthreads();
            if (tid < n) total = __fadd_rn(total, partial[tid]);
            __syncthreads();
        }
        // within the first wavefront
        for (int n = (width < 64 ? width : 64) / 2; n >= 1; n /= 2)
            total = __fadd_rn(total, __shfl_down(total, (unsigned)n));
        if (tid == 0) shared_a = n_kept > 0 ? __fdiv_rn(total, (float)n_kept) : nan32;
        __syncthreads();
        const float a = shared_a;
        const bool usable = a > 0.0f && a < __builtin_inff();
        failed = failed || !usable;
        if (usable) {
#pragma unroll
            for (int m = 0; m < IG_PER_THREAD; m++) {
                const int c = tid + m * threads;
                if (m < per_thread && c < channels && (words[c >> 6] >> (c & 63) & 1) != 0) {
                    const float2 s = ig_col[c];
                    ig_col[c] = make_float2(__fdiv_rn(s.x, a), __fdiv_rn(s.y, a));
                }
            }
        }
        if (tid == 0) mean_amplitude[p] = a;
        __syncthreads();
    }

    // ---- fill, re-rotate, scale, invert
    int n_filled = 0, gap_left = 0;
    const float2 factor = scale != nullptr ? scale[p] : make_float2(1.0f, 0.0f);
#pragma unroll
    for (int m = 0; m < IG_PER_THREAD; m++) {
        const int c = tid + m * threads;
        if (m < per_thread && c < channels) {
            float2 y = make_float2(nan32, nan32);
            if (!failed) {
                const int w = c >> 6, bit = c & 63;
                const ig_word word = words[w];
                if ((word >> bit & 1) != 0) {
                    y = ig_col[c];
                } else {
                    const ig_word lower = word & ((1ull << bit) - 1);
                    const ig_word upper = word & ~((2ull << bit) - 1);
                    const int l = lower != 0 ? 64 * w + ig_highest(lower) : w > 0 ? below[w - 1] : -1;
                    const int r = upper != 0          ? 64 * w + ig_lowest(upper)
                                  : w + 1 < n_words ? above[w + 1]
                                                    : IG_NONE_ABOVE;
                    bool got = false;
                    if (l >= 0 && r != IG_NONE_ABOVE) {
                        if (r - l - 1 <= max_gap) {
                            const float t = __fdiv_rn((float)(c - l), (float)(r - l));
                            const float2 sl = ig_col[l], sr = ig_col[r];
                            y.x = __fadd_rn(sl.x, __fmul_rn(__fsub_rn(sr.x, sl.x), t));
                            y.y = __fadd_rn(sl.y, __fmul_rn(__fsub_rn(sr.y, sl.y), t));
                            got = true;
                        }
                    } else if (l >= 0) {
                        if (c - l <= max_gap) {
                            y = ig_col[l];
                            got = true;
                        }
                    } else if (r != IG_NONE_ABOVE && r - c <= max_gap) {
                        y = ig_col[r];
                        got = true;
                    }
                    n_filled += got;
                    gap_left |= !got;
                }
                if (model != nullptr) y = ksp_cmul(y, mm[m]);
                if (scale != nullptr) y = ksp_cmul(y, factor);
                if (corrections) y = ksp_creciprocal_or_nan(y);
            }
            out[(size_t)c * out_stride + p] = y;
        }
    }

    // ---- per input
    for (int n = 32; n >= 1; n /= 2) {
        n_filled += __shfl_xor(n_filled, n);
        gap_left |= __shfl_xor(gap_left, n);
    }
    if (lane == 0) {
        wave_filled[wave] = n_filled;
        wave_gap[wave] = gap_left;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < waves; w++) {
            n_filled += wave_filled[w];
            gap_left |= wave_gap[w];
        }
        kept_out[p] = n_kept;
        filled_out[p] = n_filled;
        fill_status[p] = (uint8_t)(failed ? IG_NO_DATA : gap_left ? IG_GAP_LEFT : 0);
    }
}

extern "C" int ksp_interpolate_gains(int device, void *stream, const void *gains,
                                     const uint8_t *status, const void *model, const void *scale,
                                     void *out, int *kept, int *filled, uint8_t *fill_status,
                                     float *mean_amplitude, int channels, int n_inputs,
                                     int gains_stride, int model_stride, int out_stride,
                                     int max_gap, int smooth, int status_mask, int corrections)
{
    const ksp_plane p_gains = {"gains", gains, gains_stride, 8};
    const ksp_plane p_model = {"model", model, model_stride, 8, true};
    const ksp_plane p_out = {"out", out, out_stride, 8};
    KSP_TRY(ksp_planes_given({p_gains,
                              {"status", status, 0, 1, true},
                              p_model,
                              {"scale", scale, 0, 8, true},
                              p_out,
                              {"kept", kept, 0, 4},
                              {"filled", filled, 0, 4},
                              {"fill_status", fill_status, 0, 1},
                              {"mean_amplitude", mean_amplitude, 0, 4, true}}));
    KSP_REQUIRE(channels >= 1 && channels <= IG_MAX_CHANNELS, "channels must be 1..16384");
    KSP_REQUIRE(n_inputs >= 1, "n_inputs must be at least 1");
    KSP_REQUIRE(max_gap >= 0 && max_gap <= IG_MAX_GAP, "max_gap must be 0..16384");
    KSP_REQUIRE(smooth >= 1 && smooth <= IG_MAX_SMOOTH && smooth % 2 == 1,
                "smooth must be odd and 1..31");
    KSP_REQUIRE(status_mask >= 0 && status_mask <= 255, "status_mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_TRY(ksp_planes_hold({p_gains, p_model, p_out}, n_inputs, "n_inputs"));
    KSP_TRY(ksp_pairs_same_or_apart({p_gains, p_out}, channels, n_inputs));
    KSP_REQUIRE(model == nullptr ||
                    ksp_planes_apart(p_out, channels, n_inputs, p_model, channels, n_inputs),
                "out overlaps model");

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    constexpr auto kernel = interpolate_gains_kernel;
    KSP_TRY(ksp_lds_opt_in<kernel>(device, 8 * (size_t)IG_MAX_CHANNELS));
    const int c_pad = ksp_next_pow2(channels), threads = ig_threads(c_pad);
    const int per_thread = (channels + threads - 1) / threads;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_inputs), dim3(threads), 8 * (size_t)channels, s,
                       (const float2 *)gains, status, (const float2 *)model,
                       (const float2 *)scale, (float2 *)out, kept, filled, fill_status,
                       mean_amplitude, channels, (size_t)gains_stride, (size_t)model_stride,
                       (size_t)out_stride, c_pad, per_thread, max_gap, smooth,
                       (unsigned)status_mask, corrections);
    KSP_LAUNCH_CHECK();
    return 0;
}
