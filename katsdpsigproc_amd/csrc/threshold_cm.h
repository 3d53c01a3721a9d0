// SumThreshold along the channels of channel-major deviations ([C][stride], baselines
// contiguous), included by threshold.hip after SumParams. Flags are bit-identical to
// threshold_sum_kernel on the transposed array: the same numerical rules (see the top of
// threshold.hip), evaluated in a different order.
//
// Decomposition: one 64-thread workgroup (a single wavefront) owns 64 adjacent baselines,
// lane <-> baseline, so every channel step is one 256-byte coalesced row read and one
// 64-byte row write. The wavefront walks a channel segment [s0, s1) plus the halo
// EDGE = 2^N - N - 1 on either side ([a, b) is what it reads) and writes only [s0, s1).
// The N windows form a streaming pipeline: at step T the head of window k stands at
// channel p = T - L_k, L_k = 2^k - k - 1, and the window of size w = 2^k that ends there
// (start c = p - w + 1) is evaluated once the flags of windows 0..k-1 are final on all of
// c..p. Window k emits the final flags of windows 0..k at channel c, which is the head of
// window k+1 (L_{k+1} = L_k + w - 1). The last window emits the output at T - EDGE.
//
// Per lane and window: the flags of windows 0..k-1 over the last w channels (a w-bit
// history in registers), the channel of the last sample above the window's threshold that
// those windows left unflagged ("hot"), and the start of the last window that fired (its
// dilation reaches w channels). Deviations of the last 2^N channels sit in a per-lane ring
// in LDS ([R][64] float32, lane-contiguous, so every access is conflict-free): 4 KiB for
// 4 windows, 64 KiB for 8.
//
// A window is summed only when it holds a hot sample: w values that are all <= thr sum
// (sequentially, in float64, with monotone rounding) to at most w * thr, which equals
// float32(thr * w) or that overflows to +inf, so such a window cannot fire; a flagged
// sample stands in as thr itself and NaN is never above thr. When it holds one, the sum is
// formed exactly as the host does: float64, left to right from 0.0, flagged samples
// replaced by the window's threshold -- for every window size, so the rule "sequential
// where a sum is within its error bound of the limit" holds trivially.
// Resource use (-Rpass-analysis=kernel-resource-usage): see DESIGN.md section 4.
#pragma once

// geometry (see the launcher); -D overrides are for measuring variants only
#ifndef KSP_CM_PREFETCH
#define KSP_CM_PREFETCH 8  // channels per block of loads in flight
#endif
#ifndef KSP_CM_WAVES
#define KSP_CM_WAVES 8192  // wavefronts the launcher aims for
#endif
#ifndef KSP_CM_MIN_CORE
#define KSP_CM_MIN_CORE 64  // shortest segment core (also at least 4 halos)
#endif

namespace ksp_cm {

// flags of windows 0..k-1 on the last W channels, bit j = channel p - j
template <int W>
struct Hist {
    static constexpr int WORDS = (W + 63) / 64;
    uint64_t w[WORDS];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < WORDS; i++) w[i] = 0;
    }
    __device__ __forceinline__ void push(bool f)
    {
#pragma unroll
        for (int i = WORDS - 1; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 63);
        w[0] = (w[0] << 1) | (uint64_t)f;
    }
    __device__ __forceinline__ bool bit(int j) const
    {
        if (WORDS == 1) return (w[0] >> j) & 1;
        const uint64_t word = j < 64 ? w[0] : w[WORDS - 1];  // no dynamic register index
        return (word >> (j & 63)) & 1;
    }
};

// window K of N: state and one pipeline step
template <int K, int N>
struct Window {
    static constexpr int W = 1 << K;
    static constexpr int L = (1 << K) - K - 1;  // lag of the head behind the input channel
    static constexpr int R = 1 << N;            // ring length (> EDGE)
    Hist<W> prev;
    int hot;      // channel of the last unflagged sample > thr, or NONE
    int lasthit;  // start of the last window that fired, or NONE
    float thr;
    double limit;

    __device__ __forceinline__ void init(float t1, float scale)
    {
        prev.clear();
        hot = -(1 << 30);
        lasthit = -(1 << 30);
        thr = __fmul_rn(t1, scale);
        limit = (double)__fmul_rn(thr, (float)W);
    }

    // ring: this lane's slot of element 0; channel g is at ring[(g & (R - 1)) * 64].
    // fin: final flag of windows 0..K-1 at the head channel. Returns the final flag of
    // windows 0..K at channel T - L - W + 1.
    __device__ __forceinline__ bool step(const float *ring, int T, float x, bool fin, int a,
                                         int b)
    {
        const int p = T - L;
        prev.push(fin);
        const float dp = (L == 0) ? x : ring[(p & (R - 1)) * 64];
        if (!fin && p >= a && p < b && dp > thr) hot = p;
        const int c = p - W + 1;
        if (c >= a && p < b && hot >= c) {
            double s = 0.0;
            if (W <= 8) {
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const float v = (i == W - 1) ? dp : ring[((c + i) & (R - 1)) * 64];
                    s += (double)(prev.bit(W - 1 - i) ? thr : v);
                }
            } else {
#pragma unroll 8
                for (int i = 0; i < W; i++) {
                    const float v = ring[((c + i) & (R - 1)) * 64];
                    s += (double)(prev.bit(W - 1 - i) ? thr : v);
                }
            }
            if (s > limit) lasthit = c;
        }
        return prev.bit(W - 1) || (c - lasthit < W);
    }
};

template <int K, int N>
struct Chain {
    Window<K, N> win;
    Chain<K + 1, N> rest;
    __device__ __forceinline__ void init(float t1, const SumParams &p)
    {
        win.init(t1, p.scales[K]);
        rest.init(t1, p);
    }
    __device__ __forceinline__ bool step(const float *ring, int T, float x, bool fin, int a,
                                         int b)
    {
        return rest.step(ring, T, x, win.step(ring, T, x, fin, a, b), a, b);
    }
};

template <int N>
struct Chain<N, N> {
    __device__ __forceinline__ void init(float, const SumParams &) {}
    __device__ __forceinline__ bool step(const float *, int, float, bool fin, int, int)
    {
        return fin;
    }
};

}  // namespace ksp_cm

// Channels are read in blocks of U, the next block's loads in flight while the current one
// goes through the pipeline.
template <int N>
__global__ __launch_bounds__(64) void threshold_sum_cm_kernel(
    const float *__restrict__ dev, const float *__restrict__ noise, uint8_t *__restrict__ flags,
    int channels, int baselines, int stride, float n_sigma, SumParams params,
    uint8_t flag_value, int core)
{
    constexpr int R = 1 << N;
    constexpr int EDGE = (1 << N) - N - 1;
    constexpr int U = KSP_CM_PREFETCH;
    static_assert(R > EDGE, "the ring must hold a window's whole reach");
    __shared__ float ring_all[R * 64];
    const int lane = threadIdx.x;
    const int bl = blockIdx.x * 64 + lane;
    if (bl >= baselines) return;  // no barriers below: lanes are independent
    const int s0 = blockIdx.y * core;
    const int s1 = min(s0 + core, channels);
    const int a = max(s0 - EDGE, 0);
    const int b = min(s1 + EDGE, channels);
    const int tend = s1 + EDGE;  // steps T = a .. s1 - 1 + EDGE
    float *ring = ring_all + lane;

    ksp_cm::Chain<0, N> chain;
    chain.init(__fmul_rn(n_sigma, noise[bl]), params);

    const float *col = dev + bl;
    uint8_t *fcol = flags + bl;
    float nxt[U];
#pragma unroll
    for (int u = 0; u < U; u++) nxt[u] = (a + u < b) ? col[(size_t)(a + u) * stride] : 0.0f;
    for (int T0 = a; T0 < tend; T0 += U) {
        float cur[U];
#pragma unroll
        for (int u = 0; u < U; u++) cur[u] = nxt[u];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int g = T0 + U + u;
            nxt[u] = (g < b) ? col[(size_t)g * stride] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int T = T0 + u;
            if (T >= tend) break;
            if (N >= 2 && T < b) ring[(T & (R - 1)) * 64] = cur[u];
            const bool f = chain.step(ring, T, cur[u], false, a, b);
            const int q = T - EDGE;
            if (q >= s0 && q < s1) fcol[(size_t)q * stride] = f ? flag_value : 0;
        }
    }
}

extern "C" int ksp_threshold_sum_cm(int device, void *stream, const float *deviations,
                                    const float *noise, uint8_t *flags, int channels,
                                    int baselines, int stride, float n_sigma,
                                    const float *scales, int n_windows, int flag_value)
{
    KSP_REQUIRE(deviations != nullptr && noise != nullptr && flags != nullptr, "NULL buffer");
    KSP_REQUIRE(scales != nullptr, "scales is NULL");
    KSP_REQUIRE(channels >= 0 && baselines >= 0, "bad shape");
    KSP_REQUIRE(stride >= baselines, "stride must be >= baselines");
    KSP_REQUIRE(n_windows >= 1 && n_windows <= KSP_MAX_WINDOWS,
                "n_windows must be 1..8 (windows up to 128)");
    if (channels == 0 || baselines == 0) return 0;
    KSP_CHECK(hipSetDevice(device));
    SumParams p;
    for (int k = 0; k < KSP_MAX_WINDOWS; k++) p.scales[k] = k < n_windows ? scales[k] : 0.0f;
    const int edge = (1 << n_windows) - n_windows - 1;
    // The walk along a segment is serial per lane, so the kernel is bound by how many
    // wavefronts share the work: aim for about 8192 (8 per SIMD), with segments of at least
    // 4 halos and 64 channels so that the halo stays a small share of the reads (8192 beat
    // 2048 by 1.26x at 4096 x 8192 and 1.49x at 32768 x 4096; a deeper prefetch did nothing)
    const int groups = ksp_divup(baselines, 64);
    const int want_segments = ksp_divup(KSP_CM_WAVES, groups);
    int core = ksp_divup(channels, want_segments);
    const int min_core = 4 * edge > KSP_CM_MIN_CORE ? 4 * edge : KSP_CM_MIN_CORE;
    if (core < min_core) core = min_core;
    if (core > channels) core = channels;
    const int segments = ksp_divup(channels, core);
    KSP_REQUIRE(segments <= 65535, "too many channel segments");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(groups, segments);
    // (n_windows is 1 .. KSP_MAX_WINDOWS here)
    ksp_dispatch_exact<1, 2, 3, 4, 5, 6, 7, 8>(n_windows, [&](auto N) {
        hipLaunchKernelGGL(threshold_sum_cm_kernel<N()>, grid, dim3(64), 0, s, deviations, noise,
                           flags, channels, baselines, stride, n_sigma, p, (uint8_t)flag_value,
                           core);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
