// compress_weights: float32 weights as one byte per sample and one float32 per channel, in one
// launch (no reference counterpart). rfi/host.py CompressWeightsHost is the definition; the
// kernels reproduce it bit for bit, so every float step below is one float32 operation (the
// translation unit is built with -ffp-contract=off and correctly rounded division, and the
// quotients are written with __fdiv_rn).
//
//   per row c:      ok(w) = w > 0 && w < +inf
//                   m  = max over b of (ok(w[c][b]) ? w[c][b] : +0)
//                   wc = m / 255                                     -> weights_channel[c]
//   per sample:     t = w / wc                                       (IEEE, also for wc == 0)
//                   q = !(w > 0) ? 0 : t >= 255 ? 255 : max(1, rint(t))    -> weights8[c][b]
//
// The maximum is taken over values that are +0 or positive and finite. Their bit patterns
// order like unsigned integers, so the reduction is an integer maximum: exact, the same in any
// order, and no NaN or denormal rule of a floating-point maximum has a say.
//
// Layout. Both arrays are [channels][stride] with baselines contiguous, and a lane owns runs of
// 16 adjacent baselines (run16.h): 64 bytes of weights and 16 result bytes. A row needs its
// maximum before any byte of it can be written, so a row belongs to a team of wavefronts that
// keeps the row's weights in registers between the reduction and the quantisation; the array is
// read once. The team is chosen from the row length (cw_path, the only place that knows the
// limits):
//
//   baselines <=  1024   1 wavefront, 1 run per lane; a 256-thread workgroup holds 4 rows,
//                        and the reduction is shuffles alone (no LDS, no barrier)
//             <=  4096   4 wavefronts (256 threads), 1 run per lane
//             <= 16384  16 wavefronts (1024 threads), 1 run per lane
//             <= 32768  16 wavefronts, 2 runs per lane (32 floats held)
//             >  32768  16 wavefronts walk the row twice: once for the maximum, once to
//                       quantise (the second read of a row of at most a few hundred KiB comes
//                       from the caches more often than not)
//
// Teams of more than one wavefront exchange their maxima through LDS (one word per wavefront)
// and one barrier. Workgroups are numbered in a one-dimensional grid, so the row count is not
// bound by 65535; row bases are 64-bit. There is no workspace, no atomic and no dependence on
// the order of workgroups.
//
// The 16-byte loads apply when weights and its row starts are multiples of 16 bytes, the
// 16-byte stores when weights8 and its row starts are: one flag each.
//
// Traffic per sample: 4 bytes read, 1 written (8 read beyond 32768 baselines), and 4 bytes
// per row.
#include "launch.h"
#include "run16.h"

#define CW_ALIGNED_LOADS 1
#define CW_ALIGNED_STORES 2
// the longest row whose weights stay in registers, and the lengths below it at which the team
// changes (tests/test_gpu_compress_weights.py names the same numbers)
#define CW_WAVE_MAX 1024
#define CW_SMALL_MAX 4096
#define CW_MEDIUM_MAX 16384
#define CW_RESIDENT_MAX 32768
#define CW_LONG_THREADS 1024

// max(m, bit patterns of the weights of v that are positive and finite)
__device__ __forceinline__ unsigned cw_max(unsigned m, const float (&v)[KSP_RUN])
{
#pragma unroll
    for (int i = 0; i < KSP_RUN; i++) {
        const bool ok = v[i] > 0.0f && v[i] < __builtin_inff();
        m = max(m, ok ? __float_as_uint(v[i]) : 0u);
    }
    return m;
}

__device__ __forceinline__ unsigned cw_quantise(float w, float wc)
{
    const float t = __fdiv_rn(w, wc);
    // When w > 0, t is in [0, +inf] (wc is finite and not negative), and rint(t) held to
    // 1 .. 255 is the definition's t >= 255 ? 255 : max(1, rint(t)). Otherwise t may be
    // anything, a NaN included; the bounds make a number of it that converts, and it is dropped.
    const float q = fminf(fmaxf(rintf(t), 1.0f), 255.0f);
    return w > 0.0f ? (unsigned)q : 0u;
}

// The bytes of the weights of v, stored as far as they are `valid`
__device__ __forceinline__ void cw_store(uint8_t *out, int valid, bool wide,
                                         const float (&v)[KSP_RUN], float wc)
{
    unsigned word[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        word[q] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) word[q] |= cw_quantise(v[4 * q + k], wc) << (8 * k);
    }
    ksp_run_store_bytes(out, valid, wide, ksp_run_bytes{word[0], word[1], word[2], word[3]});
}

// The maximum over the TEAM wavefronts of a workgroup (TEAM > 1: the whole workgroup is one team)
template <int TEAM>
__device__ __forceinline__ unsigned cw_team_max(unsigned m)
{
    m = ksp_wave_max(m);
    if constexpr (TEAM > 1) {
        __shared__ unsigned wave_max[TEAM];
        if (threadIdx.x % KSP_WAVE == 0) wave_max[threadIdx.x / KSP_WAVE] = m;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TEAM; k++) m = max(m, wave_max[k]);
    }
    return m;
}

#define CW_WAVES(team) ((team) > 4 ? (team) : 4)

// A team of TEAM wavefronts per row, RUNS runs per lane, the row's weights in registers.
// Needs baselines <= TEAM * 64 * RUNS * KSP_RUN.
template <int TEAM, int RUNS>
__global__ __launch_bounds__(CW_WAVES(TEAM) * KSP_WAVE) void compress_weights_kernel(
    const float *__restrict__ weights, uint8_t *__restrict__ weights8,
    float *__restrict__ weights_channel, int channels, int baselines, long long weights_stride,
    long long weights8_stride, int aligned)
{
    constexpr int ROWS = CW_WAVES(TEAM) / TEAM;  // rows of a workgroup
    constexpr int LANES = TEAM * KSP_WAVE;       // lanes of a team
    const int lane = threadIdx.x % LANES;
    const long long row = (long long)blockIdx.x * ROWS + threadIdx.x / LANES;
    // (ROWS > 1 only with TEAM == 1, which has no barrier: whole wavefronts leave here)
    if (row >= channels) return;
    const float *w = weights + row * weights_stride;
    uint8_t *out = weights8 + row * weights8_stride;

    float v[RUNS][KSP_RUN];
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < RUNS; r++) {
        const int col0 = (r * LANES + lane) * KSP_RUN;
        ksp_run_load(w + col0, baselines - col0, aligned & CW_ALIGNED_LOADS, v[r], 0.0f);
    }
#pragma unroll
    for (int r = 0; r < RUNS; r++) m = cw_max(m, v[r]);
    m = cw_team_max<TEAM>(m);
    const float wc = __fdiv_rn(__uint_as_float(m), 255.0f);
    if (lane == 0) weights_channel[row] = wc;
#pragma unroll
    for (int r = 0; r < RUNS; r++) {
        const int col0 = (r * LANES + lane) * KSP_RUN;
        cw_store(out + col0, baselines - col0, aligned & CW_ALIGNED_STORES, v[r], wc);
    }
}

// A workgroup per row of any length: the row is read twice.
__global__ __launch_bounds__(CW_LONG_THREADS) void compress_weights_long_kernel(
    const float *__restrict__ weights, uint8_t *__restrict__ weights8,
    float *__restrict__ weights_channel, int baselines, long long weights_stride,
    long long weights8_stride, int aligned)
{
    const long long row = blockIdx.x;
    const float *w = weights + row * weights_stride;
    uint8_t *out = weights8 + row * weights8_stride;
    // (columns as 64-bit numbers: the last lanes' first column may lie beyond 2^31)
    const long long first = (long long)threadIdx.x * KSP_RUN;
    const long long step = (long long)CW_LONG_THREADS * KSP_RUN;

    unsigned m = 0;
    for (long long col0 = first; col0 < baselines; col0 += step) {
        float v[KSP_RUN];
        ksp_run_load(w + col0, (int)min((long long)KSP_RUN, baselines - col0),
                     aligned & CW_ALIGNED_LOADS, v, 0.0f);
        m = cw_max(m, v);
    }
    m = cw_team_max<CW_LONG_THREADS / KSP_WAVE>(m);
    const float wc = __fdiv_rn(__uint_as_float(m), 255.0f);
    if (threadIdx.x == 0) weights_channel[row] = wc;
    for (long long col0 = first; col0 < baselines; col0 += step) {
        const int valid = (int)min((long long)KSP_RUN, baselines - col0);
        float v[KSP_RUN];
        ksp_run_load(w + col0, valid, aligned & CW_ALIGNED_LOADS, v, 0.0f);
        cw_store(out + col0, valid, aligned & CW_ALIGNED_STORES, v, wc);
    }
}

// Which kernel takes rows of `baselines`: 0 .. 3 are the resident teams, 4 the two-pass kernel.
static int cw_path(int baselines)
{
    if (baselines <= CW_WAVE_MAX) return 0;
    if (baselines <= CW_SMALL_MAX) return 1;
    if (baselines <= CW_MEDIUM_MAX) return 2;
    if (baselines <= CW_RESIDENT_MAX) return 3;
    return 4;
}

template <int TEAM, int RUNS>
static void cw_launch(hipStream_t s, const float *weights, uint8_t *weights8,
                      float *weights_channel, int channels, int baselines, int weights_stride,
                      int weights8_stride, int aligned)
{
    constexpr int ROWS = CW_WAVES(TEAM) / TEAM;
    const dim3 grid((unsigned)(((long long)channels + ROWS - 1) / ROWS));
    hipLaunchKernelGGL((compress_weights_kernel<TEAM, RUNS>), grid,
                       dim3(CW_WAVES(TEAM) * KSP_WAVE), 0, s, weights, weights8, weights_channel,
                       channels, baselines, (long long)weights_stride, (long long)weights8_stride,
                       aligned);
}

extern "C" int ksp_compress_weights(int device, void *stream, const float *weights,
                                    uint8_t *weights8, float *weights_channel, int channels,
                                    int baselines, int weights_stride, int weights8_stride)
{
    const ksp_plane in = {"weights", weights, weights_stride, 4};
    const ksp_plane out = {"weights8", weights8, weights8_stride, 1};
    KSP_TRY(ksp_planes_given({in, out, {"weights_channel", weights_channel, 0, 4}}));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_TRY(ksp_planes_hold({in, out}, baselines, "baselines"));
    const int aligned = (ksp_planes_aligned({in}) ? CW_ALIGNED_LOADS : 0) |
                        (ksp_planes_aligned({out}) ? CW_ALIGNED_STORES : 0);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    switch (cw_path(baselines)) {
    case 0:
        cw_launch<1, 1>(s, weights, weights8, weights_channel, channels, baselines,
                        weights_stride, weights8_stride, aligned);
        break;
    case 1:
        cw_launch<4, 1>(s, weights, weights8, weights_channel, channels, baselines,
                        weights_stride, weights8_stride, aligned);
        break;
    case 2:
        cw_launch<16, 1>(s, weights, weights8, weights_channel, channels, baselines,
                         weights_stride, weights8_stride, aligned);
        break;
    case 3:
        cw_launch<16, 2>(s, weights, weights8, weights_channel, channels, baselines,
                         weights_stride, weights8_stride, aligned);
        break;
    default:
        hipLaunchKernelGGL(compress_weights_long_kernel, dim3((unsigned)channels),
                           dim3(CW_LONG_THREADS), 0, s, weights, weights8, weights_channel,
                           baselines, (long long)weights_stride, (long long)weights8_stride,
                           aligned);
    }
    KSP_LAUNCH_CHECK();
    return 0;
}
