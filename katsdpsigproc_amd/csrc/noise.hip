// Noise estimate: 1.4826 * median(|x| : x != 0) per baseline.
//
// madnz_t (baseline-major input, reference rfi/madnz_t.mako:72-87): one 256-thread
// workgroup owns one baseline; the row is read once, fully coalesced, into
// registers and the median is found by the bit-wise rank search of rank.h.
//
// madnz (channel-major input, reference rfi/madnz.mako:105-123): lane <-> baseline
// keeps the reads coalesced; like the reference kernel it re-reads the column for
// every search pass (the reference itself recommends the transposed variant,
// rfi/device.py:366), but the 16 channel phases of a workgroup make each pass a
// set of contiguous 256-byte row reads that hit in L2 after the first pass.
//
// Rows of 16385..262144 channels take madnz_t_long_kernel (madnz_long.h): one
// 1024-thread workgroup per baseline, radix select over three histogram passes.
//
// NaN input: the definition takes |x| > 0 (reference rfi/host.py:161-162), which a NaN fails
// like a zero: a NaN deviation takes no part. By its magnitude pattern a NaN sorts above
// +inf, behind every value that counts, so a kernel either loads it as +0 and counts it with
// the zeros (madnz_t_kernel: madnz_pattern below) or leaves it where it is, counts the NaN
// and takes the rank among the rest: with z zeros and k NaN among n values the median of the
// others has rank (n + z - k) / 2 in the whole row (wave_median_nonzero, madnz_kernel;
// madnz_long.h keeps both zeros and NaN out of its first histogram).
//
// Numerics (reference rfi/host.py:157-163 on float32 input): numpy.median stays in
// float32 -- even count -> float32(a + b) * 0.5 -- and the 1.4826 scale is applied
// in float64; the float32 output is that float64 product rounded once.
#include "bitplane.h"
#include "launch.h"
#include "rank.h"

#define KSP_MAD_NORMAL 1.4826

// The 31-bit pattern of |x|, 0 for a NaN (any pattern above +inf's): a NaN deviation takes no
// part in the median, exactly like a zero.
__device__ __forceinline__ unsigned madnz_pattern(unsigned bits)
{
    const unsigned p = bits & 0x7fffffffu;
    return p > 0x7f800000u ? 0u : p;
}

#include "madnz_long.h"

template <int VT>
__global__ __launch_bounds__(KSP_RANK_THREADS) void madnz_t_kernel(const float *__restrict__ in,
                                                                    float *__restrict__ noise,
                                                                    int channels, int stride)
{
    __shared__ RankScratch scratch;
    const int bl = blockIdx.x;
    const int t = threadIdx.x;
    const float *row = in + (size_t)bl * stride;
    float v[VT];
#pragma unroll
    for (int i = 0; i < VT; i++) {
        const int c = i * KSP_RANK_THREADS + t;
        // (padding is NaN, as rank.h wants it; a NaN in the data is a zero)
        v[i] = (c < channels) ? __uint_as_float(madnz_pattern(__float_as_uint(row[c])))
                              : __builtin_nanf("");
    }
    const float med = block_median_non_zero(v, channels, &scratch);
    if (t == 0) noise[bl] = (float)((double)med * KSP_MAD_NORMAL);
}

// ----------------------------------------------------------------------------
// madnz_t for rows of up to 4096 channels: ONE WAVEFRONT per baseline, lane l holds
// channels [64 l, 64 l + 64) (256 contiguous bytes per lane, 16 KiB per wavefront).
// The 31-bit patterns of |x| are transposed into 31 bit planes of 64 bits per lane
// (two in-register 32 x 32 bit transposes), after which one step of the bit-wise
// rank search is a few ANDs and population counts per lane plus DPP wave reductions
// -- two bits per step, no LDS, no barriers -- instead of a compare per value and a
// workgroup reduction per bit.
// The search itself: u[64] are the lane's 64 |x| patterns (0x7fffffff for channels that
// do not exist); returns the float32 median of the values of the row that are neither zero
// nor NaN (NaN if there are none), identical in every lane.
__device__ __forceinline__ float wave_median_nonzero(const unsigned (&u)[64], int channels)
{
    // inverted bit planes: hi[b] / hi[16 + b] = bit 16 + b of the even / odd values
    // clear; lo[...] likewise for bits 0..15
    unsigned hi[32], lo[32];
#pragma unroll
    for (int i = 0; i < 32; i++) {
        hi[i] = ~__builtin_amdgcn_perm(u[2 * i + 1], u[2 * i], 0x07060302u);
        lo[i] = ~__builtin_amdgcn_perm(u[2 * i + 1], u[2 * i], 0x05040100u);
    }
    transpose_bits32(hi);
    transpose_bits32(lo);
    auto plane = [&](int bit, int half) -> unsigned {
        return bit >= 16 ? hi[16 * half + bit - 16] : lo[16 * half + bit];
    };
    // mantissa (bits 0..22) all clear; exponent (bits 23..30) all clear / not all set
    unsigned m0 = lo[0], m1 = lo[16];
#pragma unroll
    for (int b = 1; b < 16; b++) {
        m0 &= lo[b];
        m1 &= lo[16 + b];
    }
#pragma unroll
    for (int b = 0; b < 7; b++) {
        m0 &= hi[b];
        m1 &= hi[16 + b];
    }
    unsigned e0 = hi[7], e1 = hi[23], f0 = hi[7], f1 = hi[23];
#pragma unroll
    for (int b = 8; b < 15; b++) {
        e0 &= hi[b];
        e1 &= hi[16 + b];
        f0 |= hi[b];
        f1 |= hi[16 + b];
    }
    // zeros: every one of the 31 bits clear. NaN: exponent all set, mantissa not clear; the
    // 64 * 64 - channels patterns of channels that do not exist are among them. Both counts
    // (at most 4096) share one wave reduction.
    const int packed = ksp_wave_sum_dpp(__popc(m0 & e0) + __popc(m1 & e1) +
                                        ((__popc(~(f0 | m0)) + __popc(~(f1 | m1))) << 16));
    const int zeros = packed & 0xffff;
    const int nans = (packed >> 16) - (64 * 64 - channels);
    // zeros sort first and NaN last, so the median of the values that count (non-zero, not
    // NaN) has rank (channels + zeros - nans) / 2 in the whole row (reference
    // rank.mako:261-266 for the zeros)
    const int rank2 = channels + zeros - nans;
    const int rank = rank2 / 2;
    PlaneSearch<decltype(plane)> search(rank, plane);
    // (one bit per step: measured faster than two-bit steps here as in the fused kernel)
    search.template step1<30>();
    search.template step1<29>();
    search.template step1<28>();
    search.template step1<27>();
    search.template step1<26>();
    search.template step1<25>();
    search.template step1<24>();
    search.template step1<23>();
    search.template step1<22>();
    search.template step1<21>();
    search.template step1<20>();
    search.template step1<19>();
    search.template step1<18>();
    search.template step1<17>();
    search.template step1<16>();
    search.template step1<15>();
    search.template step1<14>();
    search.template step1<13>();
    search.template step1<12>();
    search.template step1<11>();
    search.template step1<10>();
    search.template step1<9>();
    search.template step1<8>();
    search.template step1<7>();
    search.template step1<6>();
    search.template step1<5>();
    search.template step1<4>();
    search.template step1<3>();
    search.template step1<2>();
    search.template step1<1>();
    search.template step1<0>();
    const unsigned pat = search.prefix;  // pattern of the value of rank `rank`
    float result = __uint_as_float(pat);
    if (!(rank2 & 1)) {
        // even count: also the value of rank - 1 -- the same value if it occurs below
        // rank as well, else the largest value below it
        float prev = result;
        if (search.below == rank) {
            unsigned m = 0;
#pragma unroll
            for (int i = 0; i < 64; i++) m = max(m, u[i] < pat ? u[i] : 0u);
            prev = __uint_as_float(ksp_wave_max(m));
        }
        result = __fmul_rn(__fadd_rn(result, prev), 0.5f);
    }
    if (zeros + nans == channels) result = __builtin_nanf("");  // numpy: median of nothing
    return result;
}

// Self-test of the rank library (tests/test_gpu_ops.py::TestRankLibrary, the
// counterpart of reference test/test_rank.py:161-213): median of the non-zero values of
// `n` <= 16384 non-negative floats by the workgroup search (out[0]) and, for n <= 4096,
// by the wavefront bit-plane search (out[1]; else the workgroup search again).
template <int VT>
__global__ __launch_bounds__(KSP_RANK_THREADS) void selftest_median_non_zero_kernel(
    const float *__restrict__ data, int n, float *__restrict__ out)
{
    __shared__ RankScratch scratch;
    const int t = threadIdx.x;
    float v[VT];
#pragma unroll
    for (int i = 0; i < VT; i++) {
        const int c = i * KSP_RANK_THREADS + t;
        v[i] = (c < n) ? data[c] : __builtin_nanf("");
    }
    const float med = block_median_non_zero(v, n, &scratch);
    if (t == 0) out[0] = out[1] = med;
    if (n <= 4096 && t < 64) {
        unsigned u[64];
#pragma unroll
        for (int i = 0; i < 64; i++)
            u[i] = (t * 64 + i < n) ? (__float_as_uint(data[t * 64 + i]) & 0x7fffffffu) : 0x7fffffffu;
        const float w = wave_median_nonzero(u, n);
        if (t == 0) out[1] = w;
    }
}

extern "C" int ksp_selftest_median_non_zero(int device, void *stream, const float *data,
                                            float *out, int n)
{
    KSP_REQUIRE(data != nullptr && out != nullptr && n >= 1 && n <= 64 * KSP_RANK_THREADS,
                "bad arguments");
    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    // values per thread: 1 .. 64 arrive here (n was checked above)
    ksp_dispatch_ceil<4, 40, 64>(ksp_divup(n, KSP_RANK_THREADS), [&](auto VT) {
        hipLaunchKernelGGL(selftest_median_non_zero_kernel<VT()>, dim3(1), dim3(KSP_RANK_THREADS),
                           0, s, data, n, out);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void madnz_t_wave_kernel(const float *__restrict__ in,
                                                           float *__restrict__ noise, int channels,
                                                           int baselines, int stride, int vec_ok)
{
    const int lane = threadIdx.x & 63;
    const int bl = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bl >= baselines) return;  // whole wavefronts leave together
    const float *row = in + (size_t)bl * stride + lane * 64;
    // |x| patterns; channels that do not exist get the largest pattern and are never
    // reached because ranks are taken among `channels` values
    unsigned u[64];
    if (vec_ok && lane * 64 + 64 <= channels) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint4 q = *(const uint4 *)(row + 4 * i);
            u[4 * i] = q.x & 0x7fffffffu;
            u[4 * i + 1] = q.y & 0x7fffffffu;
            u[4 * i + 2] = q.z & 0x7fffffffu;
            u[4 * i + 3] = q.w & 0x7fffffffu;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 64; i++)
            u[i] = (lane * 64 + i < channels) ? (__float_as_uint(row[i]) & 0x7fffffffu) : 0x7fffffffu;
    }
    const float result = wave_median_nonzero(u, channels);
    if (lane == 0) noise[bl] = (float)((double)result * KSP_MAD_NORMAL);
}

// madnz (channel-major input) for up to 4096 channels: a 512-thread workgroup brings a
// strip of 8 adjacent baselines x all channels into LDS (32-byte row segments, the
// layout of the fused flagger: [baseline][channel], lane runs padded by 4 words), then
// each of its 8 wavefronts runs the bit-plane search on its baseline. One pass over the
// data instead of the 33 of the per-bit re-reading kernel below.
#define MADNZ_STRIP 8
#define MADNZ_RUN 68                        // 64 channels + 4 words of padding per lane
#define MADNZ_ROW (64 * MADNZ_RUN + 8)      // words per baseline
__global__ __launch_bounds__(64 * MADNZ_STRIP) void madnz_strip_kernel(
    const float *__restrict__ in, float *__restrict__ noise, int channels, int baselines, int stride)
{
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * MADNZ_STRIP;
    // cooperative load: 2 lanes x 16 B per row, 256 rows per pass
    const int q = tid & 1, r0 = tid >> 1;
    const int bq = b0 + 4 * q;
    const bool vec = (stride % 4 == 0) && ((size_t)in % 16 == 0) && (bq + 4 <= baselines);
    for (int row = r0; row < 4096; row += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < channels) {
            const float *src = in + (size_t)row * stride + bq;
            if (vec) {
                v = *(const float4 *)src;
            } else {
                if (bq < baselines) v.x = src[0];
                if (bq + 1 < baselines) v.y = src[1];
                if (bq + 2 < baselines) v.z = src[2];
                if (bq + 3 < baselines) v.w = src[3];
            }
        }
        const int idx = (row >> 6) * MADNZ_RUN + (row & 63);
        img[(4 * q + 0) * MADNZ_ROW + idx] = v.x;
        img[(4 * q + 1) * MADNZ_ROW + idx] = v.y;
        img[(4 * q + 2) * MADNZ_ROW + idx] = v.z;
        img[(4 * q + 3) * MADNZ_ROW + idx] = v.w;
    }
    __syncthreads();
    const int bl = b0 + wave;
    if (bl >= baselines) return;  // whole wavefronts leave together
    const float *run = img + wave * MADNZ_ROW + lane * MADNZ_RUN;
    unsigned u[64];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint4 w = *(const uint4 *)(run + 4 * i);
        u[4 * i] = w.x & 0x7fffffffu;
        u[4 * i + 1] = w.y & 0x7fffffffu;
        u[4 * i + 2] = w.z & 0x7fffffffu;
        u[4 * i + 3] = w.w & 0x7fffffffu;
    }
#pragma unroll
    for (int i = 0; i < 64; i++)
        if (lane * 64 + i >= channels) u[i] = 0x7fffffffu;
    const float result = wave_median_nonzero(u, channels);
    if (lane == 0) noise[bl] = (float)((double)result * KSP_MAD_NORMAL);
}

// Channel-major variant: workgroup = 64 baselines x 16 channel phases.
#define MADNZ_PHASES 16
__global__ __launch_bounds__(64 * MADNZ_PHASES) void madnz_kernel(const float *__restrict__ in,
                                                                  float *__restrict__ noise,
                                                                  int channels, int baselines,
                                                                  int stride)
{
    __shared__ int isum[MADNZ_PHASES][64];
    __shared__ float fmx[MADNZ_PHASES][64];
    const int lane = threadIdx.x & 63;
    const int phase = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane;
    const bool active = b < baselines;
    const float *col = in + (active ? b : 0);

    // counts of keys below `pivot` (and, optionally, the largest such key)
    auto count_below = [&](unsigned pivot, float *below) -> int {
        int c = 0;
        float m = 0.0f;
        for (int ch = phase; ch < channels; ch += MADNZ_PHASES) {
            const float a = fabsf(col[(size_t)ch * stride]);
            const bool lt = __float_as_uint(a) < pivot;
            c += lt;
            if (below) m = lt ? fmaxf(m, a) : m;
        }
        __syncthreads();
        isum[phase][lane] = c;
        if (below) fmx[phase][lane] = m;
        __syncthreads();
        c = 0;
        m = 0.0f;
#pragma unroll
        for (int p = 0; p < MADNZ_PHASES; p++) {
            c += isum[p][lane];
            if (below) m = fmaxf(m, fmx[p][lane]);
        }
        if (below) *below = m;
        return c;
    };

    // number of zeros = keys below the pattern of the smallest positive float; number of NaN =
    // keys not below the pattern of the smallest one. NaN sort last, so the median of the
    // values that count has rank (channels + zeros - nans) / 2 in the whole column, and no
    // pivot of the search reaches them.
    const int zeros = count_below(1u, nullptr);
    const int nans = channels - count_below(0x7f800001u, nullptr);
    const int rank2 = channels + zeros - nans;
    const int rank = rank2 / 2;
    unsigned cur = 0;
    for (int bit = 30; bit >= 0; bit--) {
        const unsigned test = cur | (1u << bit);
        const int c = count_below(test, nullptr);
        if (c <= rank) cur = test;
    }
    float result = __uint_as_float(cur);
    float below;
    const int c = count_below(cur, &below);  // barriers: every thread takes part
    if (!(rank2 & 1)) {
        const float prev = (c == rank) ? below : result;
        result = __fmul_rn(__fadd_rn(result, prev), 0.5f);
    }
    if (zeros + nans == channels) result = __builtin_nanf("");
    if (phase == 0 && active) noise[b] = (float)((double)result * KSP_MAD_NORMAL);
}

extern "C" int ksp_madnz_t(int device, void *stream, const float *in, float *noise, int channels,
                           int baselines, int stride)
{
    KSP_REQUIRE(in != nullptr && noise != nullptr, "NULL buffer");
    KSP_REQUIRE(channels > 0 && baselines >= 0 && stride >= channels, "bad shape");
    if (baselines == 0) return 0;
    if (channels > MADL_MAX_CHANNELS) {
        ksp_set_error("ksp_madnz_t: %d channels outside the supported range 1..%d", channels,
                      MADL_MAX_CHANNELS);
        return (int)hipErrorInvalidValue;
    }
    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    if (channels > 64 * KSP_RANK_THREADS) {
        // long rows (madnz_long.h): in LDS up to MADL_STAGE_MAX channels, else streamed
        const int vec = ksp_rows_aligned(in, stride, sizeof(float));
        if (channels <= MADL_STAGE_MAX) {
            const int rc = ksp_lds_opt_in<madnz_t_long_kernel<true>>(
                device, sizeof(unsigned) * MADL_STAGE_MAX);
            if (rc != 0) return rc;
            const size_t lds = sizeof(unsigned) * 4 * (size_t)ksp_divup(channels, 4);
            hipLaunchKernelGGL(madnz_t_long_kernel<true>, dim3(baselines), dim3(MADL_THREADS), lds,
                               s, in, noise, channels, stride, vec);
        } else {
            hipLaunchKernelGGL(madnz_t_long_kernel<false>, dim3(baselines), dim3(MADL_THREADS), 0,
                               s, in, noise, channels, stride, vec);
        }
        KSP_LAUNCH_CHECK();
        return 0;
    }
    if (channels > 1024 && channels <= 4096) {
        const int vec_ok = ksp_rows_aligned(in, stride, sizeof(float));
        hipLaunchKernelGGL(madnz_t_wave_kernel, dim3(ksp_divup(baselines, 4)), dim3(256), 0, s, in,
                           noise, channels, baselines, stride, vec_ok);
        KSP_LAUNCH_CHECK();
        return 0;
    }
    // channels per thread: 1 .. 4 (up to 1024 channels) and 17 .. 64 (4097 .. 16384) arrive here
    ksp_dispatch_ceil<1, 2, 4, 24, 32, 40, 64>(
        ksp_divup(channels, KSP_RANK_THREADS), [&](auto VT) {
            hipLaunchKernelGGL(madnz_t_kernel<VT()>, dim3(baselines), dim3(KSP_RANK_THREADS), 0, s,
                               in, noise, channels, stride);
        });
    KSP_LAUNCH_CHECK();
    return 0;
}

extern "C" int ksp_madnz(int device, void *stream, const float *in, float *noise, int channels,
                         int baselines, int stride)
{
    KSP_REQUIRE(in != nullptr && noise != nullptr, "NULL buffer");
    KSP_REQUIRE(channels > 0 && baselines >= 0 && stride >= baselines, "bad shape");
    if (baselines == 0) return 0;
    KSP_CHECK(hipSetDevice(device));
    if (channels <= 4096) {
        const size_t lds = sizeof(float) * MADNZ_STRIP * MADNZ_ROW;
        const int rc = ksp_lds_opt_in<madnz_strip_kernel>(device, lds);
        if (rc != 0) return rc;
        hipLaunchKernelGGL(madnz_strip_kernel, dim3(ksp_divup(baselines, MADNZ_STRIP)),
                           dim3(64 * MADNZ_STRIP), lds, (hipStream_t)stream, in, noise, channels,
                           baselines, stride);
        KSP_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(madnz_kernel, dim3(ksp_divup(baselines, 64)), dim3(64 * MADNZ_PHASES), 0,
                       (hipStream_t)stream, in, noise, channels, baselines, stride);
    KSP_LAUNCH_CHECK();
    return 0;
}
