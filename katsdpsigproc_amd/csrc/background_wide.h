// background_median_filter for wide windows (33 <= width <= 255).
//
// The narrow kernel (background.hip) keeps a whole sorted window per lane; at these widths
// that no longer fits the registers. Here one baseline's sorted window is spread over a
// group of G = 8 adjacent lanes (half a DPP row), S slots per lane, N = G * S >= width + 1
// slots in all (lane g holds slots g*S .. g*S+S-1). A step is the branch-free rule of
// median_window.h applied to the distributed array:
//   remove(out):  L[i] = s[i] < out ? s[i] : s[i+1]     (s[N] = +inf)
//   insert(in):   s[i] = med3(L[i-1], in, L[i])          (L[-1] = -inf)
// Each lane needs one value from each neighbour per step -- s[i+1] of its last slot is
// the next lane's s[0] (DPP row_shl:1), L[i-1] of its first slot is the previous lane's
// last L (row_shr:1) -- so a step costs 3*S + O(1) vector instructions per lane and
// about 3*N per sample: O(width), with no data-dependent control flow.
//
// Padding: samples that do not take part (flagged, NaN, infinite, outside the band) and the
// N - width slots beyond the window are +-inf, with #(+inf) - #(-inf) in {0, 1}, as in
// SortedWindow. N is even, so that difference is the parity of the number n of valid
// samples: with n odd the median is s[N/2 - 1], with n even the mean of s[N/2 - 1] and
// s[N/2] (slot S-1 of lane G/2 - 1 and slot 0 of lane G/2).
//
// Data flow per block of G steps: lane t of a group loads and converts the sample that
// enters at step t (each amplitude is computed once) and stores it in the baseline's
// history ring in LDS (NaN when it does not take part). The G entering and G leaving
// values of the block are then read back from the ring by every lane of the group (one
// address per group: a broadcast). After each step lane G/2 stores the two middle slots;
// at the end of the block lane t turns those of step t and the centre sample (also from
// the ring) into the output of step t, so every lane stores one output per block.
//
// Ring: R = N + G slots (>= width + G: the leaving samples of a block are never the
// entering ones, and the slots not yet written at the start still hold the NaN of the
// initialisation when they are read as leaving samples) plus a copy of its first G slots
// after the end, so that G consecutive leaving samples are always contiguous.
#pragma once
#include "launch.h"

namespace ksp_bgwide {

constexpr int G = 8;                 // lanes per baseline
constexpr int WAVES = 4;             // wavefronts per workgroup
constexpr int GROUPS = KSP_WAVE / G; // baselines per wavefront
constexpr int MAX_WIDTH = 255;

// row_shl:1 (lane i reads lane i + 1) and row_shr:1 (lane i reads lane i - 1) within a
// DPP row of 16; lanes whose source lies outside the row keep `old`
template <int CTRL>
__device__ __forceinline__ float dpp(float old, float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                 __builtin_bit_cast(int, v),
                                                                 CTRL, 0xf, 0xf, false));
}

// ring operations of one wavefront on its own LDS region: keep the compiler from moving
// LDS accesses across (the LDS executes one wavefront's accesses in order)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int S>
struct Geometry {
    static constexpr int N = G * S;      // sorted slots per baseline
    static constexpr int R = N + G;      // ring slots
    static constexpr int RING = R + G;   // ring + copy of its first G slots
    static constexpr int FLOATS = RING + 2 * G;  // + the G median pairs of a block
    static_assert(N % 2 == 0 && FLOATS % 4 == 0, "layout");
};

}  // namespace ksp_bgwide

// Grid: x = groups of WAVES * GROUPS baselines, y = channel segments of seg_len outputs.
template <int S>
__global__ __launch_bounds__(256) void background_wide_kernel(
    const void *__restrict__ in, float *__restrict__ out, const uint8_t *__restrict__ flags,
    int channels, int baselines, int stride, int flags_stride, int width, int seg_len,
    int is_amplitude, int flags_mode)
{
    using namespace ksp_bgwide;
    using Geo = Geometry<S>;
    constexpr int R = Geo::R;
    __shared__ __attribute__((aligned(16))) float lds[WAVES * GROUPS * Geo::FLOATS];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int gl = lane & (G - 1);  // lane within the group = step of the block it loads
    const int grp = lane / G;
    const int b = (blockIdx.x * WAVES + wave) * GROUPS + grp;
    const bool active = b < baselines;
    const int bb = active ? b : 0;
    const int H = width / 2;
    const int c_begin = blockIdx.y * seg_len;
    const int c_end = min(channels, c_begin + seg_len);
    const int first = c_begin - H;            // sample entering at step 0
    const int steps = c_end - c_begin + 2 * H;  // the output of step q is channel first + q - H

    float *ring = lds + (wave * GROUPS + grp) * Geo::FLOATS;
    float2 *med = reinterpret_cast<float2 *>(ring + Geo::RING);

    float pinf = __builtin_inff(), ninf = -__builtin_inff();
    asm volatile("" : "+v"(pinf), "+v"(ninf));  // keep med3 with +-inf one v_med3_f32
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < Geo::RING / G; i++) ring[i * G + gl] = nan;

    float s[S];
#pragma unroll
    for (int j = 0; j < S; j++) s[j] = gl < G / 2 ? ninf : pinf;
    bool odd = false;  // #(+inf) == #(-inf) + 1, i.e. an odd number of valid samples

    // raw sample c of the lane's baseline (clamped into the band; masked later)
    float2 z = make_float2(0.0f, 0.0f);
    bool masked = false;
    auto load = [&](int c) {
        const int cc = min(max(c, 0), channels - 1);
        const size_t idx = (size_t)cc * stride + bb;
        if (is_amplitude)
            z.x = ((const float *)in)[idx];
        else
            z = ((const float2 *)in)[idx];
        uint8_t f = 0;
        if (flags_mode == KSP_FLAGS_CHANNEL)
            f = flags[cc];
        else if (flags_mode == KSP_FLAGS_FULL)
            f = flags[(size_t)cc * flags_stride + bb];
        masked = f != 0 || c < 0 || c >= channels;
    };
    load(first + gl);
    wave_sync();

    int wslot = 0;  // ring slot of step q0 (wave-uniform)
    for (int q0 = 0; q0 < steps; q0 += G) {
        float a = is_amplitude ? z.x : ksp_abs_c64(z.x, z.y);
        if (masked) a = nan;
        if (q0 + G < steps) load(first + q0 + G + gl);  // wave-uniform; next block's sample
        ring[wslot + gl] = a;
        if (wslot == 0) ring[R + gl] = a;
        int rs = wslot - width;  // slot of the sample leaving at step q0
        if (rs < 0) rs += R;
        wave_sync();
        float vin[G], vout[G];
#pragma unroll
        for (int k = 0; k < G / 4; k++) {
            const float4 v = *reinterpret_cast<const float4 *>(ring + wslot + 4 * k);
            vin[4 * k] = v.x;
            vin[4 * k + 1] = v.y;
            vin[4 * k + 2] = v.z;
            vin[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int t = 0; t < G; t++) vout[t] = ring[rs + t];

#pragma unroll
        for (int t = 0; t < G; t++) {
            // remove: a leaving padding is taken from the +inf side when that side is ahead
            const bool out_ok = ksp_in_window(vout[t]);
            const float vo = out_ok ? vout[t] : (odd ? pinf : ninf);
            odd = (odd == out_ok);
            float nxt = dpp<0x101>(pinf, s[0]);  // row_shl:1
            nxt = gl == G - 1 ? pinf : nxt;
            float L[S];
#pragma unroll
            for (int j = 0; j < S - 1; j++) L[j] = s[j] < vo ? s[j] : s[j + 1];
            L[S - 1] = s[S - 1] < vo ? s[S - 1] : nxt;
            // insert: an entering padding goes to the side that is behind
            const bool in_ok = ksp_in_window(vin[t]);
            const float vi = in_ok ? vin[t] : (odd ? ninf : pinf);
            odd = (odd == in_ok);
            float prv = dpp<0x111>(ninf, L[S - 1]);  // row_shr:1
            prv = gl == 0 ? ninf : prv;
            s[0] = __builtin_amdgcn_fmed3f(prv, vi, L[0]);
#pragma unroll
            for (int j = 1; j < S; j++) s[j] = __builtin_amdgcn_fmed3f(L[j - 1], vi, L[j]);
            // middle slots: s[N/2 - 1] from the lane below, s[N/2] here (lane G/2); with an
            // odd count the median is the lower one alone
            const float lo = dpp<0x111>(ninf, s[S - 1]);
            if (gl == G / 2) med[t] = make_float2(lo, odd ? lo : s[0]);
        }
        wave_sync();

        // output of step q0 + gl: centre sample q0 + gl - H
        int xs = wslot + gl - H;
        if (xs < 0) xs += R;
        const float x = ring[xs];
        const float2 m = med[gl];
        const int oc = first + q0 + gl - H;
        if (active && oc >= c_begin && oc < c_end) {
            // x - (lo + hi) / 2 in float64 with the host's roundings (the sum rounded, the
            // halving exact); for an odd count lo == hi and this is x - lo rounded once
            // (NaN: a masked centre, or no finite sample in the window)
            const float d = (float)__fma_rn(-0.5, (double)m.x + (double)m.y, (double)x);
            out[(size_t)oc * stride + b] = d == d ? d : 0.0f;
        }
        wave_sync();
        wslot += G;
        if (wslot == R) wslot = 0;
    }
}

// Segments: csplit of them (0: enough for about 8192 wavefronts), of equal length and at
// least 4 * width channels each, within the band.
template <int S>
static int launch_background_wide(hipStream_t s, const void *in, float *out, const uint8_t *flags,
                                  int channels, int baselines, int stride, int flags_stride,
                                  int width, int is_amplitude, int flags_mode, int csplit)
{
    using namespace ksp_bgwide;
    constexpr int PER_BLOCK = WAVES * GROUPS;
    const int cols = ksp_divup(baselines, PER_BLOCK);
    int segs = csplit > 0 ? csplit : ksp_divup(8192, cols * WAVES);
    segs = max(1, min(segs, channels / (4 * width)));
    const int seg_len = ksp_divup(channels, segs);
    segs = ksp_divup(channels, seg_len);
    dim3 grid(cols, segs);
    hipLaunchKernelGGL(background_wide_kernel<S>, grid, dim3(64 * WAVES), 0, s, in, out, flags,
                       channels, baselines, stride, flags_stride, width, seg_len, is_amplitude,
                       flags_mode);
    KSP_LAUNCH_CHECK();
    return 0;
}

// Smallest compiled S with G * S >= width + 1: S = 5 up to width 39, then 63, 127, 191, 255.
static int launch_background_wide_any(hipStream_t s, const void *in, float *out,
                                      const uint8_t *flags, int channels, int baselines,
                                      int stride, int flags_stride, int width, int is_amplitude,
                                      int flags_mode, int csplit)
{
    int rc = 0;
    // widths 33 .. MAX_WIDTH arrive here: 5 .. 32 slots per lane
    if (ksp_dispatch_ceil<5, 8, 16, 24, 32>(ksp_divup(width + 1, ksp_bgwide::G), [&](auto S) {
            rc = launch_background_wide<S()>(s, in, out, flags, channels, baselines, stride,
                                             flags_stride, width, is_amplitude, flags_mode, csplit);
        }))
        return rc;
    ksp_set_error("ksp_background_median_filter: width %d has no compiled kernel", width);
    return (int)hipErrorInvalidValue;
}
