// band_average: per baseline and per series of channel weights, the weighted mean of the
// visibility and of its amplitude over the channels whose samples are neither NaN nor flagged
// under a mask, the weight sum, the number of samples kept and the OR of the flags of the
// series' channels: up to 8 series from one pass over the data (no reference counterpart: the
// reference's maskedsum.mako sums one series, one thread per baseline, flagged samples
// included). rfi/host.py BandAverageHost is the definition; the two kernels here reproduce it
// bit for bit, so every step is one float32 operation in the host's order (the translation
// unit is built with -ffp-contract=off and correctly rounded division, and the sums are
// written with __fmul_rn / __fadd_rn, which are never contracted).
//
// Order of the sums. The channels are cut into blocks of BA_BLOCK = 128 (the host's BLOCK: part
// of the definition, not a tuning value). Inside a block the kept samples are added in
// ascending channel order from +0.0; the block partials are added in ascending block order
// from +0.0. band_average_partial_kernel does the first for every (block, baseline) and leaves
// the partials in the workspace; band_average_combine_kernel does the second and the division.
// No atomics, no memset: every workspace word that is read was written by exactly one lane of
// the same call.
//
// Layout. data is [channels][stride] with baselines contiguous. A lane owns one baseline, a
// wavefront 64 adjacent ones (512 contiguous bytes of a row, 64 of its flags), and walks the
// rows of ONE block in ascending order with the partials of all n_series in registers, so every
// sample is read from memory once however many series there are, and |z| is computed once.
// A sample is one 8-byte load whatever the alignment of the rows: there is one path. (A variant
// whose lanes owned two baselines, with one 16-byte load per row where the rows lie on 16
// bytes, was measured and was slower: profiles/band_average.md. The lanes are what runs in
// parallel here -- the order inside a block is fixed -- and that variant has half as many.)
// Nothing beyond `baselines` of a row is read or written. The rows go in chunks through two
// sets of registers in turn: the loads of a chunk are issued before the chunk in front of it is
// added up, and nothing between the loads of a chunk uses one of them.
//
// Weights. channel_weights[k][c] is the same for the whole wavefront: the index depends on
// the block, the loop counter and k alone, so the loads are scalar. in_k = w > 0 is a scalar
// condition; a sample that is not kept is left out by a select on the addend.
//
// Workspace: float32 [n_blocks][n_series][5][baselines] -- re, im, amplitude, weight, and one
// word that holds the block's kept count (0..128) in bits 0..7 and the OR of its flags in
// bits 8..15. ksp_band_average_work_bytes gives the size: 20 bytes per (block, series,
// baseline), 1.7 % of the 9 * 128 bytes of input behind them per series.
//
// Traffic per sample: 8 + 1 bytes read once, plus 20 * n_series / 128 written and read back.
#include "launch.h"

#define BA_BLOCK 128
#define BA_MAX_SERIES 8
#define BA_MAX_CHANNELS 262144
#define BA_THREADS 256
#define BA_FIELDS 5

// Rows of a chunk; a lane has two chunks in flight. A chunk holds rows x series weights and as
// many "w > 0" conditions in scalar registers, so the rows go down as the series go up.
static constexpr int ba_chunk_rows(int ns) { return ns <= 2 ? 8 : ns <= 4 ? 4 : 2; }

// R rows of a lane as they come from memory.
template <int R>
struct BaRows {
    float2 z[R];
    unsigned f[R];
};

// Load R rows from row `c` of the array (d and fl point at the lane's baseline in row 0). A lane
// without a sample holds 1.0 (an ordinary magnitude for the amplitude's short form) and
// dereferences nothing. Nothing here uses what it loads.
template <int R, bool HAS_FLAGS>
__device__ __forceinline__ void ba_load(BaRows<R> &t, const float2 *__restrict__ d,
                                        const uint8_t *__restrict__ fl, long long c,
                                        long long data_stride, long long flags_stride, bool valid)
{
#pragma unroll
    for (int i = 0; i < R; i++) {
        t.z[i] = make_float2(1.0f, 0.0f);
        t.f[i] = 0;
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < R; i++) {
            t.z[i] = d[(c + i) * data_stride];
            if (HAS_FLAGS) t.f[i] = fl[(c + i) * flags_stride];
        }
    }
}

// The R rows of `t`, which came from row `c` of the array, into the partials.
template <int R, int NS, bool HAS_FLAGS>
__device__ __forceinline__ void ba_add(const BaRows<R> &t, const float *__restrict__ weights,
                                       long long c, long long weights_stride, unsigned mask,
                                       float (&p)[NS][4], unsigned (&cf)[NS])
{
    float a[R];
    ksp_abs_c64_rows<R>(t.z, a);  // (every lane of the wavefront is here)
#pragma unroll
    for (int i = 0; i < R; i++) {
        const float2 s = t.z[i];
        const bool ok = s.x == s.x && s.y == s.y && (t.f[i] & mask) == 0;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            const float w = weights[k * weights_stride + c + i];  // uniform: a scalar load
            const bool in_k = w > 0.0f;
            const bool kept = in_k && ok;
            p[k][0] = __fadd_rn(p[k][0], kept ? __fmul_rn(w, s.x) : 0.0f);
            p[k][1] = __fadd_rn(p[k][1], kept ? __fmul_rn(w, s.y) : 0.0f);
            p[k][2] = __fadd_rn(p[k][2], kept ? __fmul_rn(w, a[i]) : 0.0f);
            p[k][3] = __fadd_rn(p[k][3], kept ? w : 0.0f);
            cf[k] += kept ? 1u : 0u;
            if (HAS_FLAGS) cf[k] |= in_k ? t.f[i] << 8 : 0u;
        }
    }
}

// Grid: x numbers groups of BA_THREADS baselines, y the blocks of channels.
template <int NS, bool HAS_FLAGS>
__global__ __launch_bounds__(BA_THREADS) void band_average_partial_kernel(
    const float2 *__restrict__ data, const uint8_t *__restrict__ flags,
    const float *__restrict__ weights, float *__restrict__ work, int channels, int baselines,
    long long data_stride, long long flags_stride, long long weights_stride, unsigned mask)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / KSP_WAVE);
    const long long first = (long long)blockIdx.x * BA_THREADS + wave * KSP_WAVE;
    if (first >= baselines) return;  // (whole wavefronts)
    const long long b = first + threadIdx.x % KSP_WAVE;
    const bool valid = b < baselines;
    const long long c0 = (long long)blockIdx.y * BA_BLOCK;
    const int rows = (int)min((long long)BA_BLOCK, channels - c0);  // >= 1

    float p[NS][4];
    unsigned cf[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        p[k][0] = p[k][1] = p[k][2] = p[k][3] = 0.0f;
        cf[k] = 0;
    }
    const float2 *d = data + b;
    const uint8_t *fl = HAS_FLAGS ? flags + b : nullptr;
    constexpr int ROWS = ba_chunk_rows(NS);
    const int chunks = rows / ROWS;
    BaRows<ROWS> t0, t1;
    auto load = [&](BaRows<ROWS> &t, int i) __attribute__((always_inline)) {
        ba_load<ROWS, HAS_FLAGS>(t, d, fl, c0 + (long long)i * ROWS, data_stride, flags_stride,
                                 valid);
    };
    auto add = [&](const BaRows<ROWS> &t, int i) __attribute__((always_inline)) {
        ba_add<ROWS, NS, HAS_FLAGS>(t, weights, c0 + (long long)i * ROWS, weights_stride, mask, p,
                                    cf);
    };
    if (chunks > 0) {
        load(t0, 0);
        for (int i = 0;;) {
            if (i + 1 < chunks) load(t1, i + 1);
            add(t0, i);
            if (++i >= chunks) break;
            if (i + 1 < chunks) load(t0, i + 1);
            add(t1, i);
            if (++i >= chunks) break;
        }
    }
    for (int r = chunks * ROWS; r < rows; r++) {
        BaRows<1> t;
        ba_load<1, HAS_FLAGS>(t, d, fl, c0 + r, data_stride, flags_stride, valid);
        ba_add<1, NS, HAS_FLAGS>(t, weights, c0 + r, weights_stride, mask, p, cf);
    }

    if (valid) {
        float *out = work + (long long)blockIdx.y * NS * BA_FIELDS * baselines + b;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            float *q = out + (long long)k * BA_FIELDS * baselines;
#pragma unroll
            for (int t = 0; t < 4; t++) q[(long long)t * baselines] = p[k][t];
            q[4ll * baselines] = __uint_as_float(cf[k]);
        }
    }
}

// One thread per (series, baseline): the block partials in ascending order, then the means.
// Grid: x numbers groups of BA_THREADS baselines, y the series.
template <bool HAS_FLAGS>
__global__ __launch_bounds__(BA_THREADS) void band_average_combine_kernel(
    const float *__restrict__ work, float2 *__restrict__ mean, float *__restrict__ mean_amplitude,
    float *__restrict__ weight_sums, unsigned *__restrict__ counts,
    uint8_t *__restrict__ series_flags, int n_blocks, int n_series, int baselines,
    long long mean_stride, long long mean_amplitude_stride, long long weight_sums_stride,
    long long counts_stride, long long series_flags_stride)
{
    const long long b = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (b >= baselines) return;
    const int k = blockIdx.y;
    const long long field = baselines, step = (long long)n_series * BA_FIELDS * baselines;
    const float *q = work + (long long)k * BA_FIELDS * baselines + b;
    float re = 0.0f, im = 0.0f, a = 0.0f, w = 0.0f;
    unsigned count = 0, fl = 0;
#pragma unroll 4
    for (int j = 0; j < n_blocks; j++) {
        re = __fadd_rn(re, q[0]);
        im = __fadd_rn(im, q[field]);
        a = __fadd_rn(a, q[2 * field]);
        w = __fadd_rn(w, q[3 * field]);
        const unsigned cf = __float_as_uint(q[4 * field]);
        count += cf & 0xffu;
        fl |= cf >> 8;
        q += step;
    }
    const bool some = w > 0.0f;
    mean[k * mean_stride + b] =
        some ? make_float2(__fdiv_rn(re, w), __fdiv_rn(im, w)) : make_float2(0.0f, 0.0f);
    mean_amplitude[k * mean_amplitude_stride + b] = some ? __fdiv_rn(a, w) : 0.0f;
    weight_sums[k * weight_sums_stride + b] = w;
    counts[k * counts_stride + b] = count;
    if (HAS_FLAGS) series_flags[k * series_flags_stride + b] = (uint8_t)fl;
}

extern "C" size_t ksp_band_average_work_bytes(int channels, int baselines, int n_series)
{
    if (channels < 1 || baselines < 1 || n_series < 1) return 0;
    const size_t n_blocks = ((size_t)channels + BA_BLOCK - 1) / BA_BLOCK;
    return n_blocks * (size_t)n_series * BA_FIELDS * (size_t)baselines * sizeof(float);
}

extern "C" int ksp_band_average(int device, void *stream, const void *data,
                                const unsigned char *flags, const float *channel_weights,
                                void *mean, float *mean_amplitude, float *weight_sums,
                                unsigned *counts, unsigned char *series_flags, void *work_area,
                                size_t work_bytes, int channels, int baselines, int n_series,
                                int data_stride, int flags_stride, int channel_weights_stride,
                                int mean_stride, int mean_amplitude_stride,
                                int weight_sums_stride, int counts_stride,
                                int series_flags_stride, int mask)
{
    const ksp_planes in = {{"data", data, data_stride, 8}, {"flags", flags, flags_stride, 1, true}};
    const ksp_plane series = {"channel_weights", channel_weights, channel_weights_stride, 4};
    const ksp_planes out = {{"mean", mean, mean_stride, 8},
                            {"mean_amplitude", mean_amplitude, mean_amplitude_stride, 4},
                            {"weight_sums", weight_sums, weight_sums_stride, 4},
                            {"counts", counts, counts_stride, 4},
                            {"series_flags", series_flags, series_flags_stride, 1, true}};
    KSP_TRY(ksp_planes_given(in));
    KSP_TRY(ksp_planes_given({series}));
    KSP_TRY(ksp_planes_given(out));
    KSP_REQUIRE(work_area != nullptr, "work_area is NULL");
    KSP_REQUIRE((flags == nullptr) == (series_flags == nullptr),
                "flags and series_flags must both be NULL or both be given");
    KSP_REQUIRE(mask >= 0 && mask <= 255, "mask must be 0..255");
    KSP_REQUIRE(flags != nullptr || mask == 0, "mask must be 0 without flags");
    KSP_REQUIRE(channels >= 1 && channels <= BA_MAX_CHANNELS, "channels must be 1..262144");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_series >= 1 && n_series <= BA_MAX_SERIES, "n_series must be 1..8");
    KSP_TRY(ksp_planes_hold(in, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold({series}, channels, "channels"));
    KSP_TRY(ksp_planes_hold(out, baselines, "baselines"));
    KSP_REQUIRE((uintptr_t)work_area % sizeof(float) == 0, "work_area is not 4-byte aligned");
    KSP_REQUIRE(work_bytes >= ksp_band_average_work_bytes(channels, baselines, n_series),
                "work_area is smaller than ksp_band_average_work_bytes");

    const bool has_flags = flags != nullptr;
    const int n_blocks = ksp_divup(channels, BA_BLOCK);  // <= 2048: a grid's y
    // (baselines < 2^31: the count does not exceed a grid's x)
    const unsigned groups = (unsigned)(((long long)baselines + BA_THREADS - 1) / BA_THREADS);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    auto partial = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)n_blocks), dim3(BA_THREADS), 0, s,
                           (const float2 *)data, (const uint8_t *)flags, channel_weights,
                           (float *)work_area, channels, baselines, (long long)data_stride,
                           (long long)flags_stride, (long long)channel_weights_stride,
                           (unsigned)mask);
    };
    // (n_series is 1 .. 8 here)
    ksp_dispatch_exact<1, 2, 3, 4, 5, 6, 7, 8>(n_series, [&](auto NS) {
        has_flags ? partial(band_average_partial_kernel<NS(), true>)
                  : partial(band_average_partial_kernel<NS(), false>);
    });
    KSP_LAUNCH_CHECK();
    auto combine = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)n_series), dim3(BA_THREADS), 0, s,
                           (const float *)work_area, (float2 *)mean, mean_amplitude, weight_sums,
                           counts, (uint8_t *)series_flags, n_blocks, n_series, baselines,
                           (long long)mean_stride, (long long)mean_amplitude_stride,
                           (long long)weight_sums_stride, (long long)counts_stride,
                           (long long)series_flags_stride);
    };
    has_flags ? combine(band_average_combine_kernel<true>)
              : combine(band_average_combine_kernel<false>);
    KSP_LAUNCH_CHECK();
    return 0;
}
