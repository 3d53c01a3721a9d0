// range_percentiles: per channel and per range of baselines, [min, max, 25 %, 75 %, 50 %]
// ("lower" element) of the amplitudes that are neither NaN nor flagged under a mask, the
// number of them, and the OR of every flag byte of the range -- all ranges in one launch (no
// reference counterpart). rfi/host.py RangePercentilesHost is the definition; the kernel
// matches it bit for bit. With nothing left out the five values are what percentile.hip
// gives for the same column range.
//
// Keys. An amplitude is non-negative (|z| of a complex sample, or a float32 the caller
// promises to be so), so its bit pattern orders like an integer, signed or unsigned. A sample
// that takes no part -- NaN, flagged, or a slot beyond the range -- gets the key 0x7fffffff,
// which lies above +inf (0x7f800000) and is never below a search threshold. Minimum, maximum
// and the rank search are integer operations on the keys: exact, the same in any order, and no
// NaN or denormal rule of a floating-point minimum has a say. A float32 input with the sign bit
// set breaks the order and gives an unspecified value; keys are never used as addresses.
//
// Layout and teams. data is [channels][in_stride] with baselines contiguous, so a range of one
// channel is contiguous. A range belongs to a team that holds its keys in registers, chosen
// from the range's length (rp_short and the kernel's dispatch know the limits):
//
//   length <=   256   1 wavefront, 4 keys per lane; a 256-thread workgroup takes the same range
//                     of 4 adjacent channels; counts are ballots, no LDS, no barrier
//          <=  2048   4 wavefronts (the workgroup),  8 keys per lane
//          <=  4096   4 wavefronts, 16 keys per lane
//          <=  8192   4 wavefronts, 32 keys per lane
//          <= 16384   4 wavefronts, 64 keys per lane
//
// (Ranges of up to 2048 columns on a single wavefront with 8, 16 or 32 keys per lane, which
// spares them the barriers, were timed too: 15 to 30 % slower. The compares bind, not the
// barriers, and four wavefronts issue them side by side.)
//
// The three ranks (n - 1) / 4, 3 (n - 1) / 4, (n - 1) / 2 of the n kept samples share one
// 31-pass bit-wise search (as rank.h block_select3); a wavefront counts "keys below the
// threshold" with one ballot and one scalar population count per key, and the four wavefronts of
// a workgroup exchange their counts through LDS with ONE barrier per pass (two buffers in turn).
//
// Grid. One-dimensional and channel-major: the workgroups of 4 adjacent channels follow each
// other (first one per short range, then four per long range), so the rows of a channel are read
// by workgroups that are resident together. Row offsets are 64-bit, the channel count is not
// bound by 65535. No workspace, no atomics, no memset: every output element is written by
// exactly one lane.
//
// Loads. Whether a range of a row takes 16-byte loads (2 complex or 4 float samples per lane,
// with their 2 or 4 flag bytes in one load) is decided per (row, range) from the address of its
// first sample and first flag byte; otherwise, and for the ragged end, samples go one by one.
// Which lane holds which sample differs between the two, which order statistics do not see.
// Nothing outside [start, stop) of a row is read.
//
// Traffic per sample in a range: 8 (4 for amplitudes) + 1 bytes read once; 28 bytes written per
// (range, channel).
#include "launch.h"

#define RP_MAX_RANGES 16
#define RP_MAX_LENGTH 16384
#define RP_THREADS 256
#define RP_ROWS 4  // channels of a group of workgroups = wavefronts of a workgroup
// the lengths at which the team changes (tests/test_gpu_range_percentiles.py names the same)
#define RP_WAVE_MAX 256
#define RP_T8_MAX 2048
#define RP_T16_MAX 4096
#define RP_T32_MAX 8192
#define RP_EXCLUDED 0x7fffffffu

struct RpParams {
    int start[RP_MAX_RANGES];
    int length[RP_MAX_RANGES];
    int order[RP_MAX_RANGES];  // the short ranges, then the long ones
    int n_short, n_long;
};

struct RpShared {
    unsigned red[RP_ROWS][4];
    int count[2][3][RP_ROWS];
};

// Whether a range of `length` goes to a single wavefront
static inline __host__ __device__ bool rp_short(int length) { return length <= RP_WAVE_MAX; }

// Keys of CH slots of a lane, slots [first, first + CH) of its VT. `in` and `fl` point at the
// first sample and flag byte of the range in this row.
template <int CH, int LANES, bool IS_AMP, bool HAS_FLAGS>
__device__ __forceinline__ void rp_load(const void *in, const uint8_t *fl, int length, int lane,
                                        int first, bool wide, unsigned mask, unsigned *key,
                                        unsigned &any_flag)
{
    constexpr int PER = IS_AMP ? 4 : 2;  // samples of a 16-byte load
    static_assert(CH % PER == 0, "whole 16-byte loads");
    const float *inf = (const float *)in;
    const float2 *inz = (const float2 *)in;
    // a slot without a sample holds 1.0 (an ordinary magnitude for the amplitude's short form)
    float2 z[CH];
    float a[CH];
    unsigned f[CH];
    unsigned have = 0;
#pragma unroll
    for (int s = 0; s < CH; s++) {
        z[s] = make_float2(1.0f, 0.0f);
        a[s] = 1.0f;
        f[s] = 0;
    }
    auto one = [&](int s, int c) __attribute__((always_inline)) {
        if (c < length) {
            if (IS_AMP)
                a[s] = inf[c];
            else
                z[s] = inz[c];
            if (HAS_FLAGS) f[s] = fl[c];
            have |= 1u << s;
        }
    };
    if (wide) {
#pragma unroll
        for (int g = 0; g < CH / PER; g++) {
            const int c0 = ((first / PER + g) * LANES + lane) * PER;
            if (c0 + PER <= length) {
                if (IS_AMP) {
                    const float4 q = *(const float4 *)(inf + c0);
                    a[4 * g] = q.x;
                    a[4 * g + 1] = q.y;
                    a[4 * g + 2] = q.z;
                    a[4 * g + 3] = q.w;
                    if (HAS_FLAGS) {
                        const unsigned w = *(const unsigned *)(fl + c0);
#pragma unroll
                        for (int k = 0; k < 4; k++) f[4 * g + k] = (w >> (8 * k)) & 0xffu;
                    }
                } else {
                    const float4 q = *(const float4 *)(inz + c0);
                    z[2 * g] = make_float2(q.x, q.y);
                    z[2 * g + 1] = make_float2(q.z, q.w);
                    if (HAS_FLAGS) {
                        const unsigned w = *(const unsigned short *)(fl + c0);
                        f[2 * g] = w & 0xffu;
                        f[2 * g + 1] = w >> 8;
                    }
                }
                have |= ((1u << PER) - 1u) << (g * PER);
            } else {
#pragma unroll
                for (int k = 0; k < PER; k++) one(g * PER + k, c0 + k);
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < CH; s++) one(s, (first + s) * LANES + lane);
    }
    if (!IS_AMP) ksp_abs_c64_rows<CH>(z, a);  // (every lane of the wavefront is here)
#pragma unroll
    for (int s = 0; s < CH; s++) {
        const unsigned bits = __float_as_uint(a[s]);
        const bool is_nan = (bits & 0x7fffffffu) > 0x7f800000u;
        const bool kept = ((have >> s) & 1u) && !is_nan && (f[s] & mask) == 0;
        key[s] = kept ? bits : RP_EXCLUDED;
        any_flag |= f[s];
    }
}

// One range of one channel by a team of TEAM wavefronts (TEAM > 1: the whole workgroup), VT keys
// per lane. Needs length <= TEAM * 64 * VT.
template <int VT, int TEAM, bool IS_AMP, bool HAS_FLAGS>
__device__ __forceinline__ void rp_range(const void *in, const uint8_t *fl, int length,
                                         unsigned mask, RpShared *sh, float *percentiles,
                                         long long out_stride, unsigned *count_out,
                                         uint8_t *flag_out)
{
    constexpr int LANES = TEAM * KSP_WAVE;
    constexpr int CH = VT < 8 ? VT : 8;
    constexpr int PER = IS_AMP ? 4 : 2;
    const int lane = threadIdx.x % LANES;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / KSP_WAVE);
    const bool wide = (uintptr_t)in % 16 == 0 && (!HAS_FLAGS || (uintptr_t)fl % PER == 0);

    unsigned key[VT];
    unsigned any_flag = 0;
#pragma unroll
    for (int q = 0; q < VT / CH; q++)
        rp_load<CH, LANES, IS_AMP, HAS_FLAGS>(in, fl, length, lane, q * CH, wide, mask,
                                              key + q * CH, any_flag);

    int n = 0;
    unsigned lo = RP_EXCLUDED, hi = 0;
#pragma unroll
    for (int i = 0; i < VT; i++) {
        const bool kept = key[i] != RP_EXCLUDED;
        n += __builtin_popcountll(ksp_ballot(kept));
        lo = min(lo, key[i]);
        hi = max(hi, kept ? key[i] : 0u);
    }
    lo = (unsigned)__builtin_amdgcn_readlane(ksp_wave_scan_min_dpp((int)lo), 63);
    hi = (unsigned)__builtin_amdgcn_readlane(ksp_wave_scan_max_dpp((int)hi), 63);
    any_flag = ksp_wave_or_dpp(any_flag);
    if constexpr (TEAM > 1) {
        if (threadIdx.x % KSP_WAVE == 0) {
            sh->red[wave][0] = (unsigned)n;
            sh->red[wave][1] = lo;
            sh->red[wave][2] = hi;
            sh->red[wave][3] = any_flag;
        }
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < TEAM; w++) {
            n += (int)sh->red[w][0];
            lo = min(lo, sh->red[w][1]);
            hi = max(hi, sh->red[w][2]);
            any_flag |= sh->red[w][3];
        }
    }

    unsigned cur0 = 0, cur1 = 0, cur2 = 0;
    if (n > 0) {  // (the same for the whole team)
        const int r0 = (n - 1) / 4, r1 = (3 * (n - 1)) / 4, r2 = (n - 1) / 2;
        for (int bit = 30; bit >= 0; bit--) {
            const unsigned t0 = cur0 | (1u << bit), t1 = cur1 | (1u << bit),
                           t2 = cur2 | (1u << bit);
            int c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
            for (int i = 0; i < VT; i++) {
                c0 += __builtin_popcountll(ksp_ballot(key[i] < t0));
                c1 += __builtin_popcountll(ksp_ballot(key[i] < t1));
                c2 += __builtin_popcountll(ksp_ballot(key[i] < t2));
            }
            if constexpr (TEAM > 1) {
                // buffer bit & 1: a wavefront writes it again two barriers after it read it
                int(*count)[RP_ROWS] = sh->count[bit & 1];
                if (threadIdx.x % KSP_WAVE == 0) {
                    count[0][wave] = c0;
                    count[1][wave] = c1;
                    count[2][wave] = c2;
                }
                __syncthreads();
                c0 = c1 = c2 = 0;
#pragma unroll
                for (int w = 0; w < TEAM; w++) {
                    c0 += count[0][w];
                    c1 += count[1][w];
                    c2 += count[2][w];
                }
            }
            if (c0 <= r0) cur0 = t0;
            if (c1 <= r1) cur1 = t1;
            if (c2 <= r2) cur2 = t2;
        }
    } else {
        lo = hi = 0;  // five +0.0
    }
    if (lane == 0) {
        percentiles[0 * out_stride] = __uint_as_float(lo);
        percentiles[1 * out_stride] = __uint_as_float(hi);
        percentiles[2 * out_stride] = __uint_as_float(cur0);
        percentiles[3 * out_stride] = __uint_as_float(cur1);
        percentiles[4 * out_stride] = __uint_as_float(cur2);
        *count_out = (unsigned)n;
        if (HAS_FLAGS) *flag_out = (uint8_t)any_flag;
    }
}

template <bool IS_AMP, bool HAS_FLAGS>
__global__ __launch_bounds__(RP_THREADS) void range_percentiles_kernel(
    const void *__restrict__ in, const uint8_t *__restrict__ flags,
    float *__restrict__ percentiles, unsigned *__restrict__ counts,
    uint8_t *__restrict__ range_flags, int channels, long long in_stride, long long flags_stride,
    long long out_stride, long long counts_stride, long long range_flags_stride, unsigned mask,
    RpParams p)
{
    __shared__ RpShared sh;
    // workgroups of a group of RP_ROWS channels: one per short range, then RP_ROWS per long one
    const unsigned per_group = (unsigned)(p.n_short + RP_ROWS * p.n_long);
    const unsigned group = blockIdx.x / per_group;
    const int j = (int)(blockIdx.x % per_group);
    const bool is_short = j < p.n_short;
    int slot, sub;
    if (is_short) {
        slot = j;
        sub = __builtin_amdgcn_readfirstlane(threadIdx.x / KSP_WAVE);
    } else {
        slot = p.n_short + (j - p.n_short) / RP_ROWS;
        sub = (j - p.n_short) % RP_ROWS;
    }
    const long long channel = (long long)group * RP_ROWS + sub;
    // (whole wavefronts of a short range, the whole workgroup of a long one: no barrier is left
    // waiting)
    if (channel >= channels) return;
    const int r = p.order[slot];
    const int start = p.start[r], length = p.length[r];
    const void *row = IS_AMP ? (const void *)((const float *)in + channel * in_stride + start)
                             : (const void *)((const float2 *)in + channel * in_stride + start);
    const uint8_t *fl = HAS_FLAGS ? flags + channel * flags_stride + start : nullptr;
    float *pct = percentiles + (long long)r * 5 * out_stride + channel;
    unsigned *cnt = counts + r * counts_stride + channel;
    uint8_t *rf = HAS_FLAGS ? range_flags + r * range_flags_stride + channel : nullptr;
    if (is_short)
        rp_range<4, 1, IS_AMP, HAS_FLAGS>(row, fl, length, mask, &sh, pct, out_stride, cnt, rf);
    else if (length <= RP_T8_MAX)
        rp_range<8, RP_ROWS, IS_AMP, HAS_FLAGS>(row, fl, length, mask, &sh, pct, out_stride, cnt, rf);
    else if (length <= RP_T16_MAX)
        rp_range<16, RP_ROWS, IS_AMP, HAS_FLAGS>(row, fl, length, mask, &sh, pct, out_stride, cnt, rf);
    else if (length <= RP_T32_MAX)
        rp_range<32, RP_ROWS, IS_AMP, HAS_FLAGS>(row, fl, length, mask, &sh, pct, out_stride, cnt, rf);
    else
        rp_range<64, RP_ROWS, IS_AMP, HAS_FLAGS>(row, fl, length, mask, &sh, pct, out_stride, cnt, rf);
}

extern "C" int ksp_range_percentiles(int device, void *stream, const void *in,
                                     const unsigned char *flags, float *percentiles,
                                     unsigned *counts, unsigned char *range_flags, int channels,
                                     int baselines, int in_stride, int flags_stride,
                                     int out_stride, int counts_stride, int range_flags_stride,
                                     const int *ranges, int n_ranges, int is_amplitude, int mask)
{
    // (percentiles goes by two names: its row stride is out_stride)
    const ksp_planes by_baseline = {{"in", in, in_stride, is_amplitude ? 4 : 8},
                                    {"flags", flags, flags_stride, 1, true}};
    const ksp_planes by_channel = {{"out", percentiles, out_stride, 4},
                                   {"counts", counts, counts_stride, 4},
                                   {"range_flags", range_flags, range_flags_stride, 1, true}};
    KSP_TRY(ksp_planes_given(by_baseline));
    KSP_REQUIRE(percentiles != nullptr, "percentiles is NULL");
    KSP_TRY(ksp_planes_given(by_channel));
    KSP_REQUIRE(ranges != nullptr, "ranges is NULL");
    KSP_REQUIRE((flags == nullptr) == (range_flags == nullptr),
                "flags and range_flags must both be NULL or both be given");
    KSP_REQUIRE(mask >= 0 && mask <= 255, "mask must be 0..255");
    KSP_REQUIRE(flags != nullptr || mask == 0, "mask must be 0 without flags");
    KSP_REQUIRE(channels >= 0, "channels must not be negative");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_ranges >= 1 && n_ranges <= RP_MAX_RANGES, "n_ranges must be 1..16");
    KSP_TRY(ksp_planes_hold(by_baseline, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold(by_channel, channels, "channels"));
    RpParams p = {};
    for (int r = 0; r < n_ranges; r++) {
        const int start = ranges[2 * r], stop = ranges[2 * r + 1];
        KSP_REQUIRE(start >= 0 && start <= stop && stop <= baselines,
                    "a range must satisfy 0 <= start <= stop <= baselines");
        KSP_REQUIRE(stop - start <= RP_MAX_LENGTH, "a range is longer than 16384 columns");
        p.start[r] = start;
        p.length[r] = stop - start;
    }
    for (int r = 0; r < n_ranges; r++)
        if (rp_short(p.length[r])) p.order[p.n_short++] = r;
    for (int r = 0; r < n_ranges; r++)
        if (!rp_short(p.length[r])) p.order[p.n_short + p.n_long++] = r;
    const long long groups = ((long long)channels + RP_ROWS - 1) / RP_ROWS;
    const long long blocks = groups * (p.n_short + RP_ROWS * p.n_long);
    KSP_REQUIRE(blocks <= 0x7fffffffLL, "channels times ranges exceeds the grid");
    if (channels == 0) return 0;

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(RP_THREADS);
    const bool has_flags = flags != nullptr;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, in, (const uint8_t *)flags, percentiles,
                           counts, (uint8_t *)range_flags, channels, (long long)in_stride,
                           (long long)flags_stride, (long long)out_stride,
                           (long long)counts_stride, (long long)range_flags_stride,
                           (unsigned)mask, p);
    };
    if (is_amplitude)
        has_flags ? launch(range_percentiles_kernel<true, true>)
                  : launch(range_percentiles_kernel<true, false>);
    else
        has_flags ? launch(range_percentiles_kernel<false, true>)
                  : launch(range_percentiles_kernel<false, false>);
    KSP_LAUNCH_CHECK();
    return 0;
}
