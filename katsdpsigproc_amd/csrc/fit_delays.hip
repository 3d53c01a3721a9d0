// fit_delays: per input, the delay and phase whose phasor best matches the gains of
// ksp_solve_gains across the band, and that phasor for every channel, in one launch (no
// reference counterpart). rfi/host.py FitDelaysHost is the definition; the kernel reproduces it
// bit for bit, so every float32 step of the transform and every float64 step of the refinement
// is one operation, rounded once (the translation unit is built with -ffp-contract=off, and the
// steps are written with __fmul_rn / __fadd_rn / __fsub_rn and __dmul_rn / __dadd_rn /
// __dsub_rn, which are never contracted; the float64 division and square root are the
// compiler's correctly rounded expansions).
//
//   per input p, with x[c] = gains[c][p] where both parts are finite and status[c] & mask == 0,
//   else 0, and 0 for c = channels .. n_fft - 1:
//   coarse, float32: X = the radix-2 decimation-in-time transform of x (bit reversal, then the
//     stages s = 1 .. log2 n_fft, half = 2^(s-1), butterfly (j, j + half) with the twiddle
//     (float32(co), float32(-si)), (co, si) = cos_sin((j mod half) / 2^s):
//       bt = (b.re tw.re - b.im tw.im, b.re tw.im + b.im tw.re);  a' = a + bt;  b' = a - bt)
//     P[k] = re re + im im;  k0 = the lowest k of the largest P that is not NaN
//   refinement, float64, from nu = k0 / n_fft, `refine` times:
//     e = (x.re co + x.im si, x.im co - x.re si), (co, si) = cos_sin(c nu), per kept channel
//     D0 = sum e;  D1 = sum c e;  D2 = sum (c c) e       (halving trees over Cpad terms)
//     num = D1.im D0.re - D1.re D0.im
//     den = 6.283185307179586 ((D1.re D1.re + D1.im D1.im) - (D2.re D0.re + D2.im D0.im))
//     step = num / den;  den < 0 and |step| <= 1 / n_fft ? nu -= step : bit 1, stop
//   results from D0 at the final nu: m = |D0|, phasor = D0 / m rounded to float32,
//     amplitude = m / n_kept, delay = (nu - rint(nu)) / channel_width,
//     model[c][p] = phasor exp(2 pi i c nu) for every channel of the band.
//
// One workgroup per input; n_fft complex64 of dynamic LDS hold the transform (128 KiB at
// 16384). The workgroup has n_fft / 8 threads, at least 64 and at most 1024. The column is read
// with 8-byte loads at a stride of gains_stride elements: all workgroups read the same lines,
// which therefore come from L2. Thread g loads the FD_RUN = 8 elements that the bit reversal
// puts at 8 g .. 8 g + 7 (channels rev(g) + {0, 4, 2, 6, 1, 5, 3, 7} n_fft / 8, of which the
// odd multiples lie beyond the band and are never read), does the stages with half = 1, 2, 4
// on them in registers, where power-of-two strides on 8-byte words would collide on banks, and
// stores them. The later stages run in LDS, a barrier apart: consecutive threads take
// consecutive j, 2-way conflicts at half = 8 and 16 and none above. A transform of 4 runs both
// stages in LDS. The twiddles are evaluated with the float64 series of cal_math.h
// (ksp_cos_sin_turns, which is cos_sin above).
//
// After the peak search the transform is dead and its LDS carries the sums across wavefronts.
// The refinement reads x again from gains (L2): thread i owns channels i, i + T, i + 2 T, ...,
// so the upper levels of a tree are thread-local (visited in bit-reversed order with one
// partial sum per level), the next ones go through LDS, the last six through lane shuffles.
// Every decision is taken from the same values by every thread: uniform over the workgroup.
// model is written by the same workgroup, 8-byte stores at a stride of model_stride elements.
// No atomics, no workspace, no dependence on the order of workgroups. Padding is neither read
// nor written.
#include <cmath>

#include "cal_math.h"
#include "launch.h"

#define FD_MIN_FFT 4
#define FD_MAX_FFT 16384
#define FD_MAX_REFINE 8
#define FD_RUN 8
#define FD_MAX_THREADS 1024
#define FD_NO_FIT 1
#define FD_STEP_REJECTED 2

static int fd_threads(int n_fft)
{
    const int t = n_fft / FD_RUN;
    return t < 64 ? 64 : t > FD_MAX_THREADS ? FD_MAX_THREADS : t;
}
// Dynamic LDS: the transform, or (only larger for the smallest transforms) the six sums of
// the upper half of the threads
static size_t fd_lds_bytes(int n_fft)
{
    const size_t transform = 8 * (size_t)n_fft, sums = 6 * 8 * (size_t)(fd_threads(n_fft) / 2);
    return transform > sums ? transform : sums;
}

// The twiddle of butterfly j of stage s: j < 2^(s-1), so the quotient is exact
__device__ __forceinline__ float2 fd_twiddle(int j, int s)
{
    double co, si;
    ksp_cos_sin_turns(__dmul_rn((double)j, 1.0 / (double)(1 << s)), co, si);
    return make_float2((float)co, (float)-si);
}

__device__ __forceinline__ void fd_butterfly(float2 &a, float2 &b, float2 tw)
{
    const float2 bt = ksp_cmul(b, tw), a0 = a;
    a = make_float2(__fadd_rn(a0.x, bt.x), __fadd_rn(a0.y, bt.y));
    b = make_float2(__fsub_rn(a0.x, bt.x), __fsub_rn(a0.y, bt.y));
}

// x[c] of input p, and whether the channel is kept (c < channels)
template <bool HAS_S>
__device__ __forceinline__ float2 fd_load(const float2 *gains, const uint8_t *status,
                                          long long gains_stride, int p, int c, unsigned mask,
                                          bool &kept)
{
    const float2 g = gains[c * gains_stride + p];
    kept = __builtin_isfinite(g.x) && __builtin_isfinite(g.y);
    if (HAS_S) kept = kept && (status[c] & mask) == 0;
    return kept ? g : make_float2(0.0f, 0.0f);
}

struct fd_sums {
    double v[6];  // D0.re, D0.im, D1.re, D1.im, D2.re, D2.im
};

__device__ __forceinline__ fd_sums fd_add(const fd_sums &a, const fd_sums &b)
{
    fd_sums r;
#pragma unroll
    for (int i = 0; i < 6; i++) r.v[i] = __dadd_rn(a.v[i], b.v[i]);
    return r;
}

// D0, D1, D2 at nu, the same in every thread. `wide` is the dynamic LDS, `shared` six doubles.
template <bool HAS_S>
__device__ fd_sums fd_pass(const float2 *gains, const uint8_t *status, long long gains_stride,
                           int p, int channels, int c_pad, unsigned mask, double nu, double *wide,
                           double *shared)
{
    const int tid = threadIdx.x, threads = blockDim.x;
    // the thread's own channels tid + m threads, m < 2^levels, in bit-reversed order: the sums
    // of a level wait in part[level] for their partner (a binary counter's carries)
    const int width = c_pad < threads ? c_pad : threads;  // terms after the thread-local levels
    int levels = 0;
    while ((width << levels) < c_pad) levels++;  // (at most 3)
    fd_sums p0, p1, p2, total;
    for (int q = 0; q < (1 << levels); q++) {
        const int m = levels > 0 ? (int)(__brev((unsigned)q) >> (32 - levels)) : 0;
        const int c = tid + m * threads;
        fd_sums cur;
#pragma unroll
        for (int i = 0; i < 6; i++) cur.v[i] = 0.0;
        if (c < channels) {
            bool kept;
            const float2 x = fd_load<HAS_S>(gains, status, gains_stride, p, c, mask, kept);
            if (kept) {
                const double cd = (double)c, xr = (double)x.x, xi = (double)x.y;
                double co, si;
                ksp_cos_sin_turns(__dmul_rn(cd, nu), co, si);
                const double er = __dadd_rn(__dmul_rn(xr, co), __dmul_rn(xi, si));
                const double ei = __dsub_rn(__dmul_rn(xi, co), __dmul_rn(xr, si));
                const double c2 = __dmul_rn(cd, cd);
                cur.v[0] = er;
                cur.v[1] = ei;
                cur.v[2] = __dmul_rn(cd, er);
                cur.v[3] = __dmul_rn(cd, ei);
                cur.v[4] = __dmul_rn(c2, er);
                cur.v[5] = __dmul_rn(c2, ei);
            }
        }
        if ((q & 1) == 0) {
            p0 = cur;
        } else {
            cur = fd_add(p0, cur);
            if ((q & 2) == 0) {
                p1 = cur;
            } else {
                cur = fd_add(p1, cur);
                if ((q & 4) == 0)
                    p2 = cur;
                else
                    cur = fd_add(p2, cur);
            }
        }
        total = cur;  // (the last one is the sum of all)
    }
    // across wavefronts: the upper half hands its sums to the lower half
    fd_sums *slots = reinterpret_cast<fd_sums *>(wide);
    for (int n = width / 2; n >= 64; n /= 2) {
        if (tid >= n && tid < 2 * n) slots[tid - n] = total;
        __syncthreads();
        if (tid < n) total = fd_add(total, slots[tid]);
        __syncthreads();
    }
    // within the first wavefront
    for (int n = (width < 64 ? width : 64) / 2; n >= 1; n /= 2) {
        fd_sums other;
#pragma unroll
        for (int i = 0; i < 6; i++) other.v[i] = __shfl_down(total.v[i], (unsigned)n);
        total = fd_add(total, other);
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) shared[i] = total.v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; i++) total.v[i] = shared[i];
    __syncthreads();  // (shared is written again in the next pass)
    return total;
}

template <bool HAS_S, bool HAS_M>
__global__ __launch_bounds__(FD_MAX_THREADS) void fit_delays_kernel(
    const float2 *__restrict__ gains, const uint8_t *__restrict__ status,
    double *__restrict__ delays, float2 *__restrict__ phasors, float *__restrict__ amplitudes,
    uint8_t *__restrict__ fit_status, float2 *__restrict__ model, int channels,
    long long gains_stride, long long model_stride, int n_fft, int log2_fft, int c_pad, int refine,
    unsigned mask, int corrections, double channel_width)
{
    extern __shared__ double fd_lds[];
    __shared__ double shared[6];
    __shared__ float best_p[FD_MAX_THREADS / 64];
    __shared__ int best_k[FD_MAX_THREADS / 64], counts[FD_MAX_THREADS / 64];
    float2 *X = reinterpret_cast<float2 *>(fd_lds);
    const int tid = threadIdx.x, threads = blockDim.x;
    const int p = blockIdx.x;

    // ---- load in bit-reversed order, the first stages in registers
    int n_kept = 0;
    int first_stage = 1;
    if (n_fft >= FD_RUN) {
        first_stage = 4;
        const int eighth = n_fft / FD_RUN;
        for (int g = tid; g < eighth; g += threads) {
            const int base = log2_fft > 3 ? (int)(__brev((unsigned)g) >> (35 - log2_fft)) : 0;
            float2 v[FD_RUN];
#pragma unroll
            for (int m = 0; m < FD_RUN; m++) {
                const int rev3 = ((m & 1) << 2) | (m & 2) | (m >> 2);
                const int c = base + rev3 * eighth;
                bool kept = false;
                v[m] = make_float2(0.0f, 0.0f);
                if (c < channels)
                    v[m] = fd_load<HAS_S>(gains, status, gains_stride, p, c, mask, kept);
                n_kept += kept;
            }
#pragma unroll
            for (int s = 1; s <= 3; s++) {
                const int half = 1 << (s - 1);
#pragma unroll
                for (int b = 0; b < FD_RUN / 2; b++) {
                    const int j = b & (half - 1), at = ((b >> (s - 1)) << s) + j;
                    fd_butterfly(v[at], v[at + half], fd_twiddle(j, s));
                }
            }
#pragma unroll
            for (int m = 0; m < FD_RUN; m++) X[g * FD_RUN + m] = v[m];
        }
    } else {
        // n_fft = 4: channels 0 and 1 (at most) to positions 0 and 2
        if (tid < n_fft) {
            const int c = ((tid & 1) << 1) | (tid >> 1);
            bool kept = false;
            float2 v = make_float2(0.0f, 0.0f);
            if (c < channels) v = fd_load<HAS_S>(gains, status, gains_stride, p, c, mask, kept);
            n_kept += kept;
            X[tid] = v;
        }
    }
    __syncthreads();

    // ---- the later stages in LDS
    for (int s = first_stage; s <= log2_fft; s++) {
        const int half = 1 << (s - 1);
        // up to half = threads every butterfly of a thread has the same j
        const bool one_twiddle = half <= threads;
        float2 tw = fd_twiddle(tid & (half - 1), s);
        for (int b = tid; b < n_fft / 2; b += threads) {
            const int j = b & (half - 1), at = ((b >> (s - 1)) << s) + j;
            float2 lo = X[at], hi = X[at + half];
            if (!one_twiddle) tw = fd_twiddle(j, s);
            fd_butterfly(lo, hi, tw);
            X[at] = lo;
            X[at + half] = hi;
        }
        __syncthreads();
    }

    // ---- the peak: the largest power that is not NaN, at its lowest index
    float peak = -1.0f;  // (no power is negative)
    int k0 = 0x7fffffff;
    for (int k = tid; k < n_fft; k += threads) {
        const float power = ksp_norm2(X[k]);
        if (power > peak) {  // (k ascends within a thread)
            peak = power;
            k0 = k;
        }
    }
    for (int n = 32; n >= 1; n /= 2) {
        const float other_p = __shfl_xor(peak, n);
        const int other_k = __shfl_xor(k0, n);
        n_kept += __shfl_xor(n_kept, n);
        if (other_p > peak || (other_p == peak && other_k < k0)) {
            peak = other_p;
            k0 = other_k;
        }
    }
    if ((tid & 63) == 0) {
        best_p[tid >> 6] = peak;
        best_k[tid >> 6] = k0;
        counts[tid >> 6] = n_kept;
    }
    __syncthreads();  // (and everyone is done with the transform)
    peak = best_p[0];
    k0 = best_k[0];
    n_kept = counts[0];
    for (int w = 1; w < threads / 64; w++) {
        const float other_p = best_p[w];
        const int other_k = best_k[w];
        n_kept += counts[w];
        if (other_p > peak || (other_p == peak && other_k < k0)) {
            peak = other_p;
            k0 = other_k;
        }
    }

    // ---- refine
    bool no_fit = n_kept < 2 || !(peak > 0.0f && peak < __builtin_inff());
    unsigned bits = 0;
    double nu = 0.0, ph_re = 0.0, ph_im = 0.0, m = 0.0;
    if (!no_fit) {
        nu = __dmul_rn((double)k0, 1.0 / (double)n_fft);
        const double limit = 1.0 / (double)n_fft;
        for (int it = 0; it < refine; it++) {
            const fd_sums d = fd_pass<HAS_S>(gains, status, gains_stride, p, channels, c_pad, mask,
                                             nu, fd_lds, shared);
            const double num = __dsub_rn(__dmul_rn(d.v[3], d.v[0]), __dmul_rn(d.v[2], d.v[1]));
            const double den = __dmul_rn(
                6.283185307179586,
                __dsub_rn(__dadd_rn(__dmul_rn(d.v[2], d.v[2]), __dmul_rn(d.v[3], d.v[3])),
                          __dadd_rn(__dmul_rn(d.v[4], d.v[0]), __dmul_rn(d.v[5], d.v[1]))));
            const double step = num / den;
            if (den < 0.0 && fabs(step) <= limit) {
                nu = __dsub_rn(nu, step);
            } else {
                bits |= FD_STEP_REJECTED;
                break;
            }
        }
        const fd_sums d = fd_pass<HAS_S>(gains, status, gains_stride, p, channels, c_pad, mask, nu,
                                         fd_lds, shared);
        m = __builtin_sqrt(__dadd_rn(__dmul_rn(d.v[0], d.v[0]), __dmul_rn(d.v[1], d.v[1])));
        no_fit = !(m > 0.0 && m < (double)__builtin_inff());
        if (!no_fit) {
            ph_re = d.v[0] / m;
            ph_im = d.v[1] / m;
        }
    }
    if (no_fit) bits |= FD_NO_FIT;

    // ---- results
    const float nan32 = __builtin_nanf("");
    const float2 phasor = no_fit ? make_float2(nan32, nan32) : make_float2((float)ph_re, (float)ph_im);
    if (tid == 0) {
        delays[p] = no_fit ? __builtin_nan("") : __dsub_rn(nu, rint(nu)) / channel_width;
        phasors[p] = phasor;
        amplitudes[p] = no_fit ? nan32 : (float)(m / (double)n_kept);
        fit_status[p] = (uint8_t)bits;
    }
    if (HAS_M) {
        const double wide_re = (double)phasor.x, wide_im = (double)phasor.y;
        for (int c = tid; c < channels; c += threads) {
            float2 out = make_float2(nan32, nan32);
            if (!no_fit) {
                double co, si;
                ksp_cos_sin_turns(__dmul_rn((double)c, nu), co, si);
                out.x = (float)__dsub_rn(__dmul_rn(wide_re, co), __dmul_rn(wide_im, si));
                out.y = (float)__dadd_rn(__dmul_rn(wide_re, si), __dmul_rn(wide_im, co));
                if (corrections) out.y = -out.y;
            }
            model[c * model_stride + p] = out;
        }
    }
}

extern "C" int ksp_fit_delays(int device, void *stream, const void *gains, const uint8_t *status,
                              double *delays, void *phasors, float *amplitudes,
                              uint8_t *fit_status, void *model, int channels, int n_inputs,
                              int gains_stride, int model_stride, int n_fft, int refine,
                              int status_mask, int corrections, double channel_width)
{
    const ksp_plane p_gains = {"gains", gains, gains_stride, 8};
    const ksp_plane p_model = {"model", model, model_stride, 8, true};
    KSP_TRY(ksp_planes_given({p_gains,
                              {"status", status, 0, 1, true},
                              {"delays", delays, 0, 8},
                              {"phasors", phasors, 0, 8},
                              {"amplitudes", amplitudes, 0, 4},
                              {"fit_status", fit_status, 0, 1}}));
    KSP_REQUIRE(channels >= 1 && channels <= FD_MAX_FFT / 2, "channels must be 1..8192");
    KSP_REQUIRE(n_inputs >= 1, "n_inputs must be at least 1");
    KSP_REQUIRE(n_fft >= FD_MIN_FFT && n_fft <= FD_MAX_FFT && (n_fft & (n_fft - 1)) == 0,
                "n_fft must be a power of two in 4..16384");
    KSP_REQUIRE(n_fft >= 2 * channels, "n_fft must be at least twice the channels");
    KSP_REQUIRE(refine >= 0 && refine <= FD_MAX_REFINE, "refine must be 0..8");
    KSP_REQUIRE(status_mask >= 0 && status_mask <= 255, "status_mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_REQUIRE(std::isfinite(channel_width) && channel_width != 0.0,
                "channel_width must be finite and not 0");
    KSP_TRY(ksp_planes_hold({p_gains, p_model}, n_inputs, "n_inputs"));
    KSP_REQUIRE(model == nullptr || ksp_planes_apart(p_model, channels, n_inputs, p_gains,
                                                     channels, n_inputs),
                "model overlaps gains");

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    int log2_fft = 0;
    while ((1 << log2_fft) < n_fft) log2_fft++;
    const int c_pad = ksp_next_pow2(channels);
    const int variant = (status != nullptr ? 1 : 0) | (model != nullptr ? 2 : 0);
    int rc = 0;
    ksp_dispatch_exact<0, 1, 2, 3>(variant, [&](auto V) {
        constexpr auto kernel = fit_delays_kernel<(V() & 1) != 0, (V() & 2) != 0>;
        rc = ksp_lds_opt_in<kernel>(device, fd_lds_bytes(FD_MAX_FFT));
        if (rc != 0) return;
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_inputs), dim3(fd_threads(n_fft)),
                           fd_lds_bytes(n_fft), s, (const float2 *)gains, status, delays,
                           (float2 *)phasors, amplitudes, fit_status, (float2 *)model, channels,
                           (long long)gains_stride, (long long)model_stride, n_fft, log2_fft,
                           c_pad, refine, (unsigned)status_mask, corrections, channel_width);
    });
    KSP_TRY(rc);
    KSP_LAUNCH_CHECK();
    return 0;
}
