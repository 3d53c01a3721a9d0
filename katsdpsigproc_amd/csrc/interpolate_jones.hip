// interpolate_jones: per antenna, the 2x2 Jones matrices of ksp_solve_jones filled across the
// channels the solver left without a matrix, in one launch (no reference counterpart): the 2x2
// counterpart of interpolate_gains.hip. Per feed row the delay model of ksp_fit_delays is
// divided out, each of the four elements gets a running mean over the kept channels, the
// antenna's mean amplitude is normalised, gaps of up to max_gap channels are interpolated
// linearly (held at the ends of the band), the model and a band-wide gain per feed are
// multiplied back in, and optionally the matrix is inverted. rfi/host.py InterpolateJonesHost
// is the definition; the kernel reproduces it bit for bit, so every step is one float32
// operation, rounded once (-ffp-contract=off, __f*_rn, correctly rounded division and square
// root, as interpolate_gains.hip).
//
//   per antenna a, with z[i][k] = jones[c][2a + i][k] and m_i = model[c][2a + i]:
//   kept[c]: all eight floats of z finite, status[c] & mask == 0, all four floats of m_0, m_1
//     finite: one mask per antenna;  n_kept counts them;  none: bit 0, the antenna is NaN
//   d[i][k] = z[i][k] conj(m_i)                                          (z without model)
//   s[i][k][c] = the running mean of interpolate_gains.hip, per element, over the same kept
//     channels and with the same count for all four                      (d for smooth = 1)
//   a = (halving tree over Cpad terms of sqrt(((n00 + n01) + (n10 + n11)) 0.5), nik = the
//     squared modulus of s[i][k], +0 where not kept) / float(n_kept);  a in (0, inf): all
//     eight floats of s are divided by a, else bit 0
//   fill: per element as interpolate_gains.hip, with one l, r and t for the four elements
//   y[i][k] = y[i][k] m_i, then y[i][k] scale[2a + i]
//   corrections: D = y00 y11 - y01 y10, q = |D|^2, inv = q > 0 ? (D.re / q, -D.im / q) : NaN,
//     y = [[y11 inv, -(y01 inv)], [-(y10 inv), y00 inv]]
//
// One workgroup per antenna, with the threads, the ballot words of kept channels, the max/min
// scans and the halving tree of interpolate_gains.hip. The four elements go one after the other
// through ONE column of `channels` complex64 in dynamic LDS (128 KiB at 16384, where four
// columns would not fit), at every size:
//   pass 0  reads the antenna's whole input for the kept mask (before the first store);
//   pass 1  (only with smooth > 1 or the normalisation) per element: d into the column, the
//           running mean out of it, s stored to `out`; then the amplitude's terms from the four
//           s of each channel, read back;
//   pass 2  per element: s (from `out`, or d straight from `jones` when pass 1 was not needed)
//           divided by a into the column, then every channel filled from the column,
//           re-rotated, scaled and stored to `out`;
//   pass 3  (only with corrections) per channel: the four elements read back and inverted.
// Thread i owns channels i, i + T, i + 2 T, ... in every pass, so what it reads back from `out`
// it wrote itself, and an element's input is read by the thread that later overwrites it, before
// it does: `out` may be `jones`. The model and the scale are read again where they are needed
// (they come from L2), which keeps the kernel without register arrays beyond the amplitude's
// terms. Every barrier is reached by every thread: the decisions around them (smooth, the
// normalisation, `failed`, corrections) are taken from kernel arguments and from values all
// threads read from LDS. Row offsets are size_t. No atomics, no workspace, no dependence on the
// order of workgroups. Padding is neither read nor written.
//
// jones_diagonal: gains[c][p] = jones[c][p][p % 2], a copy of bits, one thread per (c, p).
#include "cal_math.h"
#include "launch.h"

#define IJ_MAX_CHANNELS 16384
#define IJ_MAX_INPUTS 2048
#define IJ_MAX_GAP 16384
#define IJ_MAX_SMOOTH 31
#define IJ_MAX_THREADS 1024
#define IJ_PER_THREAD (IJ_MAX_CHANNELS / IJ_MAX_THREADS)
#define IJ_MAX_WORDS (IJ_MAX_CHANNELS / 64)
#define IJ_SCAN_WAVES (IJ_MAX_WORDS / 64)
#define IJ_NO_DATA 1
#define IJ_GAP_LEFT 2
#define IJ_NONE_ABOVE 0x7fffffff
#define JD_THREADS 256

typedef unsigned long long ij_word;

static int ij_threads(int c_pad)
{
    return c_pad < 64 ? 64 : c_pad > IJ_MAX_THREADS ? IJ_MAX_THREADS : c_pad;
}

__device__ __forceinline__ int ij_highest(ij_word word) { return 63 - __clzll((long long)word); }
__device__ __forceinline__ int ij_lowest(ij_word word) { return __ffsll(word) - 1; }
__device__ __forceinline__ bool ij_bit(const ij_word *words, int c)
{
    return (words[c >> 6] >> (c & 63) & 1) != 0;
}

__global__ __launch_bounds__(IJ_MAX_THREADS) void interpolate_jones_kernel(
    const float2 *jones, const uint8_t *__restrict__ status, const float2 *__restrict__ model,
    const float2 *__restrict__ scale, float2 *out, int *__restrict__ kept_out,
    int *__restrict__ filled_out, uint8_t *__restrict__ fill_status,
    float *__restrict__ mean_amplitude, int channels, size_t jones_stride, size_t model_stride,
    size_t out_stride, int c_pad, int per_thread, int max_gap, int smooth, unsigned mask,
    int corrections)
{
    extern __shared__ float2 ij_col[];
    __shared__ ij_word words[IJ_MAX_WORDS];
    __shared__ int below[IJ_MAX_WORDS], above[IJ_MAX_WORDS];
    __shared__ int wave_lo[IJ_SCAN_WAVES], wave_hi[IJ_SCAN_WAVES], wave_kept[IJ_SCAN_WAVES];
    __shared__ float partial[IJ_MAX_THREADS / 2];
    __shared__ int wave_filled[IJ_MAX_THREADS / 64], wave_gap[IJ_MAX_THREADS / 64];
    __shared__ float shared_a;
    const int tid = threadIdx.x, threads = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int waves = threads >> 6;
    const size_t ant = blockIdx.x;
    const float nan32 = __builtin_nanf("");
    // element e = 2 i + k of channel c: jones[(c jones_stride + 2 ant) 2 + e] in complex64
    const float2 *const in0 = jones + 4 * ant;
    float2 *const out0 = out + 4 * ant;
    const float2 *const model0 = model != nullptr ? model + 2 * ant : nullptr;

    // ---- pass 0: the words of `kept`, from everything the antenna reads
#pragma unroll 1
    for (int m = 0; m < per_thread; m++) {
        const int c = tid + m * threads;
        bool keep = false;
        if (c < channels) {
            const float2 *z = in0 + 2 * ((size_t)c * jones_stride);
            keep = ksp_cfinite(z[0]) && ksp_cfinite(z[1]) && ksp_cfinite(z[2]) &&
                   ksp_cfinite(z[3]);
            if (status != nullptr) keep = keep && (status[c] & mask) == 0;
            if (model != nullptr) {
                const float2 *mc = model0 + (size_t)c * model_stride;
                keep = keep && ksp_cfinite(mc[0]) && ksp_cfinite(mc[1]);
            }
        }
        const ij_word ballot = __ballot(keep);
        if (lane == 0) words[m * waves + wave] = ballot;
    }
    __syncthreads();

    // ---- per word: the nearest kept channel at or below its end and at or above its start
    const int n_words = per_thread * waves;
    const int scan_waves = waves < IJ_SCAN_WAVES ? waves : IJ_SCAN_WAVES;
    int lo = -1, hi = IJ_NONE_ABOVE;
    if (tid < IJ_MAX_WORDS) {  // (whole wavefronts)
        const ij_word word = tid < n_words ? words[tid] : 0;
        int count = __popcll(word);
        if (word != 0) {
            lo = 64 * tid + ij_highest(word);
            hi = 64 * tid + ij_lowest(word);
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
    if (tid < IJ_MAX_WORDS) {
        for (int w = 0; w < wave; w++) lo = wave_lo[w] > lo ? wave_lo[w] : lo;
        for (int w = wave + 1; w < scan_waves; w++) hi = wave_hi[w] < hi ? wave_hi[w] : hi;
        below[tid] = lo;
        above[tid] = hi;
    }
    int n_kept = 0;
    for (int w = 0; w < scan_waves; w++) n_kept += wave_kept[w];
    __syncthreads();

    // ---- pass 1: the running mean of every element
    const bool normalise = mean_amplitude != nullptr;
    const bool first_pass = smooth > 1 || normalise;  // (the same for every thread)
    if (first_pass) {
        const int reach = smooth >> 1;
#pragma unroll 1
        for (int e = 0; e < 4; e++) {
#pragma unroll 1
            for (int m = 0; m < per_thread; m++) {
                const int c = tid + m * threads;
                if (c < channels && ij_bit(words, c)) {
                    float2 d = in0[2 * ((size_t)c * jones_stride) + e];
                    if (model != nullptr)
                        d = ksp_cmul_conj(d, model0[(size_t)c * model_stride + (e >> 1)]);
                    ij_col[c] = d;
                }
            }
            __syncthreads();
#pragma unroll 1
            for (int m = 0; m < per_thread; m++) {
                const int c = tid + m * threads;
                if (c < channels && ij_bit(words, c)) {
                    float2 s = ij_col[c];
                    if (smooth > 1) {
                        const int first = c - reach < 0 ? 0 : c - reach;
                        const int last = c + reach > channels - 1 ? channels - 1 : c + reach;
                        float re = 0.0f, im = 0.0f;
                        int n = 0;
                        for (int j = first; j <= last; j++)
                            if (ij_bit(words, j)) {
                                const float2 d = ij_col[j];
                                re = __fadd_rn(re, d.x);
                                im = __fadd_rn(im, d.y);
                                n++;
                            }
                        s = make_float2(__fdiv_rn(re, (float)n), __fdiv_rn(im, (float)n));
                    }
                    out0[2 * ((size_t)c * out_stride) + e] = s;
                }
            }
            __syncthreads();
        }
    }

    // ---- the mean amplitude
    bool failed = n_kept == 0;
    float a = 1.0f;
    if (normalise) {
        float term[IJ_PER_THREAD];
#pragma unroll
        for (int m = 0; m < IJ_PER_THREAD; m++) {
            term[m] = 0.0f;
            const int c = tid + m * threads;
            if (m < per_thread && c < channels && ij_bit(words, c)) {
                // (the four s of the channel, which this thread stored in pass 1)
                const float2 *s = out0 + 2 * ((size_t)c * out_stride);
                const float upper = __fadd_rn(ksp_norm2(s[0]), ksp_norm2(s[1]));
                const float lower = __fadd_rn(ksp_norm2(s[2]), ksp_norm2(s[3]));
                term[m] = __builtin_sqrtf(__fmul_rn(__fadd_rn(upper, lower), 0.5f));
            }
        }
        // the levels of the tree whose two terms belong to one thread: i + m T with i + (m + n) T
        const int local_terms = c_pad > threads ? c_pad / threads : 1;
#pragma unroll
        for (int n = IJ_PER_THREAD / 2; n >= 1; n /= 2)
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
        a = shared_a;
        failed = failed || !(a > 0.0f && a < __builtin_inff());
        if (tid == 0) mean_amplitude[ant] = a;
    }

    // ---- pass 2: fill, re-rotate, scale
    int n_filled = 0, gap_left = 0;
    if (failed) {  // (the same for every thread)
        for (int m = 0; m < per_thread; m++) {
            const int c = tid + m * threads;
            if (c < channels) {
                float2 *y = out0 + 2 * ((size_t)c * out_stride);
                y[0] = y[1] = y[2] = y[3] = make_float2(nan32, nan32);
            }
        }
    } else {
#pragma unroll 1
        for (int e = 0; e < 4; e++) {
            const float2 factor = scale != nullptr ? scale[2 * ant + (e >> 1)]
                                                   : make_float2(1.0f, 0.0f);
            for (int m = 0; m < per_thread; m++) {
                const int c = tid + m * threads;
                if (c < channels && ij_bit(words, c)) {
                    float2 s;
                    if (first_pass) {
                        s = out0[2 * ((size_t)c * out_stride) + e];
                    } else {
                        s = in0[2 * ((size_t)c * jones_stride) + e];
                        if (model != nullptr)
                            s = ksp_cmul_conj(s, model0[(size_t)c * model_stride + (e >> 1)]);
                    }
                    if (normalise) s = make_float2(__fdiv_rn(s.x, a), __fdiv_rn(s.y, a));
                    ij_col[c] = s;
                }
            }
            __syncthreads();
            for (int m = 0; m < per_thread; m++) {
                const int c = tid + m * threads;
                if (c < channels) {
                    float2 y = make_float2(nan32, nan32);
                    const int w = c >> 6, bit = c & 63;
                    const ij_word word = words[w];
                    if ((word >> bit & 1) != 0) {
                        y = ij_col[c];
                    } else {
                        const ij_word under = word & ((1ull << bit) - 1);
                        const ij_word over = word & ~((2ull << bit) - 1);
                        const int l = under != 0 ? 64 * w + ij_highest(under)
                                      : w > 0    ? below[w - 1]
                                                 : -1;
                        const int r = over != 0           ? 64 * w + ij_lowest(over)
                                      : w + 1 < n_words ? above[w + 1]
                                                        : IJ_NONE_ABOVE;
                        bool got = false;
                        if (l >= 0 && r != IJ_NONE_ABOVE) {
                            if (r - l - 1 <= max_gap) {
                                const float t = __fdiv_rn((float)(c - l), (float)(r - l));
                                const float2 sl = ij_col[l], sr = ij_col[r];
                                y.x = __fadd_rn(sl.x, __fmul_rn(__fsub_rn(sr.x, sl.x), t));
                                y.y = __fadd_rn(sl.y, __fmul_rn(__fsub_rn(sr.y, sl.y), t));
                                got = true;
                            }
                        } else if (l >= 0) {
                            if (c - l <= max_gap) {
                                y = ij_col[l];
                                got = true;
                            }
                        } else if (r != IJ_NONE_ABOVE && r - c <= max_gap) {
                            y = ij_col[r];
                            got = true;
                        }
                        if (e == 0) {  // (one l, r for the four elements: counted once)
                            n_filled += got;
                            gap_left |= !got;
                        }
                    }
                    if (model != nullptr)
                        y = ksp_cmul(y, model0[(size_t)c * model_stride + (e >> 1)]);
                    if (scale != nullptr) y = ksp_cmul(y, factor);
                    out0[2 * ((size_t)c * out_stride) + e] = y;
                }
            }
            __syncthreads();
        }

        // ---- pass 3: the inverse, from what this thread has just stored
        if (corrections) {
            for (int m = 0; m < per_thread; m++) {
                const int c = tid + m * threads;
                if (c < channels) {
                    float2 *y = out0 + 2 * ((size_t)c * out_stride);
                    const float2 ja = y[0], jb = y[1], jc = y[2], jd = y[3];
                    // (a NaN `inverse` leaves NaN in all four elements)
                    const float2 inverse = ksp_creciprocal_or_nan(ksp_det2(ja, jb, jc, jd));
                    float2 x0, y0, x1, y1;
                    ksp_adj2_row_times(ja, jb, jc, jd, inverse, false, x0, y0);
                    ksp_adj2_row_times(ja, jb, jc, jd, inverse, true, x1, y1);
                    y[0] = x0;
                    y[1] = y0;
                    y[2] = x1;
                    y[3] = y1;
                }
            }
        }
    }

    // ---- per antenna
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
        kept_out[ant] = n_kept;
        filled_out[ant] = n_filled;
        fill_status[ant] = (uint8_t)(failed ? IJ_NO_DATA : gap_left ? IJ_GAP_LEFT : 0);
    }
}

__global__ __launch_bounds__(JD_THREADS) void jones_diagonal_kernel(
    const float2 *__restrict__ jones, float2 *__restrict__ gains, size_t total, int n_inputs,
    size_t jones_stride, size_t gains_stride)
{
    const size_t i = (size_t)blockIdx.x * JD_THREADS + threadIdx.x;
    if (i >= total) return;
    const size_t c = i / (size_t)n_inputs, p = i % (size_t)n_inputs;
    gains[c * gains_stride + p] = jones[2 * (c * jones_stride + p) + (p & 1)];
}

extern "C" int ksp_interpolate_jones(int device, void *stream, const void *jones,
                                     const uint8_t *status, const void *model, const void *scale,
                                     void *out, int *kept, int *filled, uint8_t *fill_status,
                                     float *mean_amplitude, int channels, int n_inputs,
                                     int jones_stride, int model_stride, int out_stride,
                                     int max_gap, int smooth, int status_mask, int corrections)
{
    // (an element of jones and of out is a row of two complex64)
    const ksp_plane p_jones = {"jones", jones, jones_stride, 16};
    const ksp_plane p_model = {"model", model, model_stride, 8, true};
    const ksp_plane p_out = {"out", out, out_stride, 16};
    KSP_TRY(ksp_planes_given({p_jones,
                              {"status", status, 0, 1, true},
                              p_model,
                              {"scale", scale, 0, 8, true},
                              p_out,
                              {"kept", kept, 0, 4},
                              {"filled", filled, 0, 4},
                              {"fill_status", fill_status, 0, 1},
                              {"mean_amplitude", mean_amplitude, 0, 4, true}}));
    KSP_REQUIRE(channels >= 1 && channels <= IJ_MAX_CHANNELS, "channels must be 1..16384");
    KSP_REQUIRE(n_inputs >= 2 && n_inputs <= IJ_MAX_INPUTS && n_inputs % 2 == 0,
                "n_inputs must be even and 2..2048");
    KSP_REQUIRE(max_gap >= 0 && max_gap <= IJ_MAX_GAP, "max_gap must be 0..16384");
    KSP_REQUIRE(smooth >= 1 && smooth <= IJ_MAX_SMOOTH && smooth % 2 == 1,
                "smooth must be odd and 1..31");
    KSP_REQUIRE(status_mask >= 0 && status_mask <= 255, "status_mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_TRY(ksp_planes_hold({p_jones, p_model, p_out}, n_inputs, "n_inputs"));
    KSP_TRY(ksp_pairs_same_or_apart({p_jones, p_out}, channels, n_inputs));
    KSP_REQUIRE(model == nullptr ||
                    ksp_planes_apart(p_out, channels, n_inputs, p_model, channels, n_inputs),
                "out overlaps model");

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    constexpr auto kernel = interpolate_jones_kernel;
    KSP_TRY(ksp_lds_opt_in<kernel>(device, 8 * (size_t)IJ_MAX_CHANNELS));
    const int c_pad = ksp_next_pow2(channels), threads = ij_threads(c_pad);
    const int per_thread = (channels + threads - 1) / threads;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_inputs / 2)), dim3(threads),
                       8 * (size_t)channels, s, (const float2 *)jones, status,
                       (const float2 *)model, (const float2 *)scale, (float2 *)out, kept, filled,
                       fill_status, mean_amplitude, channels, (size_t)jones_stride,
                       (size_t)model_stride, (size_t)out_stride, c_pad, per_thread, max_gap,
                       smooth, (unsigned)status_mask, corrections);
    KSP_LAUNCH_CHECK();
    return 0;
}

extern "C" int ksp_jones_diagonal(int device, void *stream, const void *jones, void *gains,
                                  int channels, int n_inputs, int jones_stride, int gains_stride)
{
    const ksp_plane p_jones = {"jones", jones, jones_stride, 16};
    const ksp_plane p_gains = {"gains", gains, gains_stride, 8};
    KSP_TRY(ksp_planes_given({p_jones, p_gains}));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(n_inputs >= 1, "n_inputs must be at least 1");
    KSP_TRY(ksp_planes_hold({p_jones, p_gains}, n_inputs, "n_inputs"));
    KSP_REQUIRE(ksp_planes_apart(p_jones, channels, n_inputs, p_gains, channels, n_inputs),
                "gains overlaps jones");
    const size_t total = (size_t)channels * (size_t)n_inputs;
    const size_t groups = (total + JD_THREADS - 1) / JD_THREADS;
    KSP_REQUIRE(groups <= 0x7fffffffull, "array too large for one launch");

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jones_diagonal_kernel, dim3((unsigned)groups), dim3(JD_THREADS), 0, s,
                       (const float2 *)jones, (float2 *)gains, total, n_inputs,
                       (size_t)jones_stride, (size_t)gains_stride);
    KSP_LAUNCH_CHECK();
    return 0;
}
