// prepare: a correlator's integer dump as the inputs of the flagging chain, in one launch (no
// reference counterpart). rfi/host.py PrepareHost is the definition; the kernel reproduces
// it bit for bit, so every float step below is one float32 operation in the host's order
// (the translation unit is built with -ffp-contract=off and correctly rounded division, and
// the products are written with __fmul_rn, the quotient with __fdiv_rn).
//
//   per channel c and output baseline j:
//     s = source[j];  valid = 0 <= s < in_baselines;  (re, im) = vis_in[c][valid ? s : 0]
//     lost = !valid || re == -2^31
//     vis = lost ? (0, 0) : (float(re) * scale, float(im) * scale)
//     input_flags = channel_flags[c] | (lost ? lost_flag : 0)
//   with weights:
//     power(k) = valid k && vis_in[c][k].re != -2^31 ? float(vis_in[c][k].re) * scale : 0
//     pa, pb = power(auto_source[j][0]), power(auto_source[j][1]);  d = pa * pb
//     weights = pa > 0 && pb > 0 && d > 0 ? weight_scale / d : 0
//
// Indices are data. An index is compared with the range as an unsigned number and replaced
// by 0 when it is outside (in_baselines >= 1, so element 0 of a row exists); only then is an
// address formed from it, and the load is issued whether the index was valid or not: no lane
// branches around a load, and any int32 in source or auto_source has the result above.
//
// Layout. The outputs are [channels][stride] with baselines contiguous, as in average.hip,
// and a lane owns a run of PREP_RUN = 16 adjacent output baselines: 16 flag bytes (one
// 16-byte store), 128 bytes of visibilities (8 stores) and 64 bytes of weights (4). Its 16
// source entries are four 16-byte loads, its 32 auto_source entries eight. These are the same
// for every row, so a lane keeps them (range-checked, with the validity as a bit mask) and
// walks PREP_ROWS adjacent rows with them: four with weights (48 registers of indices, loaded
// once for four rows of output instead of 192 bytes again for every 208 written), two
// without. The register count does not depend on the number (the row loop is not unrolled);
// the numbers are the fastest of 1, 2, 4 and 8 at 4096 x 32768 (profiles/prepare.md). Items (a
// run of a group of rows) are numbered group after group and dealt to the threads of a
// one-dimensional grid, so the row count is not bound by the 65535 of the other grid
// dimensions; row bases are 64-bit. Per row the inputs are sixteen 8-byte gathers from the row
// of vis_in and, with weights, thirty-two 4-byte gathers of real parts, which in practice hit
// a handful of addresses (the autocorrelations of the antennas) over and over.
//
// The 16-byte paths apply when every output pointer and row start, source and auto_source
// are multiples of 16 bytes and vis_in is a multiple of 8 (its row stride is in pairs). The
// ragged run at the end of a row, and every run of a call that is not aligned so, go element
// by element with 4-byte loads. Padding of the outputs is never written, padding of vis_in
// never read. (The run of run16.h, by hand: written on its helpers, with the arithmetic stated
// once, the instances without weights were slower on the 16-byte path, profiles/run16.md.)
//
// Traffic per sample: 8 bytes gathered, 8 + 1 written, 4 more with weights.
#include <limits.h>

#include "launch.h"

#define PREP_THREADS 256
#define PREP_RUN 16
#define PREP_ROWS(has_w) ((has_w) ? 4 : 2)

// `index` if it is inside 0 .. n - 1, else 0; `ok` says which
__device__ __forceinline__ int prep_clamp(int index, int n, bool &ok)
{
    ok = (unsigned)index < (unsigned)n;
    return ok ? index : 0;
}

__device__ __forceinline__ float prep_power(int re, bool ok, float scale)
{
    return (ok && re != INT_MIN) ? __fmul_rn((float)re, scale) : 0.0f;
}

__device__ __forceinline__ float prep_weight(float pa, float pb, float weight_scale)
{
    const float d = __fmul_rn(pa, pb);
    const bool some = pa > 0.0f && pb > 0.0f && d > 0.0f;
    // (the divisor of a sample that gets no weight is 1: the quotient is then not used)
    const float q = __fdiv_rn(weight_scale, some ? d : 1.0f);
    return some ? q : 0.0f;
}

// The instances with weights take 191 registers (two waves per SIMD): 48 indices, the 64 words
// of a row's gathers and the 64-bit addresses of the loads in flight. Held to three waves they
// were slower (profiles/prepare.md), held to four they spill: no occupancy bound.
template <bool HAS_CF, bool HAS_W>
__global__ __launch_bounds__(PREP_THREADS) void prepare_kernel(
    const int *__restrict__ vis_in, const int *__restrict__ source,
    const int *__restrict__ auto_source, const uint8_t *__restrict__ channel_flags,
    float2 *__restrict__ vis, uint8_t *__restrict__ input_flags, float *__restrict__ weights,
    long long items, int runs_per_row, int channels, int in_baselines, int baselines,
    long long vis_in_stride, long long vis_stride, long long input_flags_stride,
    long long weights_stride, float scale, float weight_scale, unsigned lost_flag, int aligned)
{
    const long long item = (long long)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (item >= items) return;
    const long long group = item / runs_per_row;
    const int col0 = (int)(item - group * runs_per_row) * PREP_RUN;
    const int valid = min(PREP_RUN, baselines - col0);  // >= 1
    constexpr int ROWS = PREP_ROWS(HAS_W);
    const long long row0 = group * ROWS;
    const int rows = (int)min((long long)ROWS, channels - row0);  // >= 1

    if (aligned && valid == PREP_RUN) {
        // the indices of the run, once for all its rows
        int s[PREP_RUN], a[HAS_W ? 2 * PREP_RUN : 1];
        unsigned s_ok = 0, a_ok = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int4 t = reinterpret_cast<const int4 *>(source + col0)[q];
            const int tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bool ok;
                s[4 * q + k] = prep_clamp(tt[k], in_baselines, ok);
                s_ok |= (unsigned)ok << (4 * q + k);
            }
        }
        if (HAS_W) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int4 t = reinterpret_cast<const int4 *>(auto_source + 2 * col0)[q];
                const int tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    bool ok;
                    a[4 * q + k] = prep_clamp(tt[k], in_baselines, ok);
                    a_ok |= (unsigned)ok << (4 * q + k);
                }
            }
        }
        for (int r = 0; r < rows; r++) {
            const long long row = row0 + r;
            const int *in = vis_in + 2 * row * vis_in_stride;
            float2 *v = vis + row * vis_stride + col0;
            uint8_t *fl = input_flags + row * input_flags_stride + col0;
            const unsigned cf = HAS_CF ? channel_flags[row] : 0u;
            int2 z[PREP_RUN];
#pragma unroll
            for (int i = 0; i < PREP_RUN; i++) z[i] = reinterpret_cast<const int2 *>(in)[s[i]];
            int p[HAS_W ? 2 * PREP_RUN : 1];
            if (HAS_W) {
#pragma unroll
                for (int i = 0; i < 2 * PREP_RUN; i++) p[i] = in[2 * (long long)a[i]];
            }
            unsigned fw[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float o[8];
                fw[q] = cf * 0x01010101u;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = 4 * q + k;
                    const bool lost = !((s_ok >> i) & 1u) || z[i].x == INT_MIN;
                    o[2 * k] = lost ? 0.0f : __fmul_rn((float)z[i].x, scale);
                    o[2 * k + 1] = lost ? 0.0f : __fmul_rn((float)z[i].y, scale);
                    fw[q] |= (lost ? lost_flag : 0u) << (8 * k);
                }
                reinterpret_cast<float4 *>(v)[2 * q] = make_float4(o[0], o[1], o[2], o[3]);
                reinterpret_cast<float4 *>(v)[2 * q + 1] = make_float4(o[4], o[5], o[6], o[7]);
            }
            *reinterpret_cast<uint4 *>(fl) = make_uint4(fw[0], fw[1], fw[2], fw[3]);
            if (HAS_W) {
                float *w = weights + row * weights_stride + col0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float o[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = 2 * (4 * q + k);
                        const float pa = prep_power(p[i], (a_ok >> i) & 1u, scale);
                        const float pb = prep_power(p[i + 1], (a_ok >> (i + 1)) & 1u, scale);
                        o[k] = prep_weight(pa, pb, weight_scale);
                    }
                    reinterpret_cast<float4 *>(w)[q] = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    } else {
        for (int i = 0; i < valid; i++) {
            bool ok, ok_a = false, ok_b = false;
            const int si = prep_clamp(source[col0 + i], in_baselines, ok);
            int ia = 0, ib = 0;
            if (HAS_W) {
                ia = prep_clamp(auto_source[2 * (col0 + i)], in_baselines, ok_a);
                ib = prep_clamp(auto_source[2 * (col0 + i) + 1], in_baselines, ok_b);
            }
            for (int r = 0; r < rows; r++) {
                const long long row = row0 + r;
                const int *in = vis_in + 2 * row * vis_in_stride;
                const int re = in[2 * (long long)si], im = in[2 * (long long)si + 1];
                const bool lost = !ok || re == INT_MIN;
                float2 z;
                z.x = lost ? 0.0f : __fmul_rn((float)re, scale);
                z.y = lost ? 0.0f : __fmul_rn((float)im, scale);
                vis[row * vis_stride + col0 + i] = z;
                const unsigned cf = HAS_CF ? channel_flags[row] : 0u;
                input_flags[row * input_flags_stride + col0 + i] =
                    (uint8_t)(cf | (lost ? lost_flag : 0u));
                if (HAS_W) {
                    const float pa = prep_power(in[2 * (long long)ia], ok_a, scale);
                    const float pb = prep_power(in[2 * (long long)ib], ok_b, scale);
                    weights[row * weights_stride + col0 + i] = prep_weight(pa, pb, weight_scale);
                }
            }
        }
    }
}

static bool prep_positive(float x) { return x > 0.0f && x <= 3.402823466e+38f; }

extern "C" int ksp_prepare(int device, void *stream, const int32_t *vis_in, const int32_t *source,
                           const int32_t *auto_source, const uint8_t *channel_flags, void *vis,
                           uint8_t *input_flags, float *weights, int channels, int in_baselines,
                           int baselines, int vis_in_stride, int vis_stride,
                           int input_flags_stride, int weights_stride, float scale,
                           float weight_scale, int lost_flag)
{
    KSP_REQUIRE(vis_in != nullptr, "vis_in is NULL");
    KSP_REQUIRE(source != nullptr, "source is NULL");
    KSP_REQUIRE(vis != nullptr, "vis is NULL");
    KSP_REQUIRE(input_flags != nullptr, "input_flags is NULL");
    KSP_REQUIRE((auto_source == nullptr) == (weights == nullptr),
                "auto_source and weights must both be given or both be NULL");
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(in_baselines >= 1, "in_baselines must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(vis_in_stride >= in_baselines, "vis_in_stride is smaller than in_baselines");
    KSP_REQUIRE(vis_stride >= baselines, "vis_stride is smaller than baselines");
    KSP_REQUIRE(input_flags_stride >= baselines, "input_flags_stride is smaller than baselines");
    KSP_REQUIRE(weights == nullptr || weights_stride >= baselines,
                "weights_stride is smaller than baselines");
    KSP_REQUIRE(prep_positive(scale), "scale must be finite and positive");
    KSP_REQUIRE(weights == nullptr || prep_positive(weight_scale),
                "weight_scale must be finite and positive");
    KSP_REQUIRE(lost_flag >= 1 && lost_flag <= 255, "lost_flag must be 1..255");
    const int runs_per_row = ksp_divup(baselines, PREP_RUN);
    const int rows_per_item = PREP_ROWS(weights != nullptr);
    const long long row_groups = ((long long)channels + rows_per_item - 1) / rows_per_item;
    const long long items = row_groups * runs_per_row;
    const long long groups = (items + PREP_THREADS - 1) / PREP_THREADS;
    KSP_REQUIRE(groups <= 0x7fffffffll, "array too large for one launch");
    const int aligned =
        (uintptr_t)vis_in % 8 == 0 && ksp_rows_aligned(source, 0, 4) &&
        ksp_rows_aligned_if_given(auto_source, 0, 4) &&
        ksp_rows_aligned(vis, vis_stride, 8) &&
        ksp_rows_aligned(input_flags, input_flags_stride, 1) &&
        ksp_rows_aligned_if_given(weights, weights_stride, 4);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)groups);
    ksp_dispatch_exact<0, 1, 2, 3>(
        (channel_flags != nullptr ? 1 : 0) + (weights != nullptr ? 2 : 0), [&](auto V) {
            hipLaunchKernelGGL((prepare_kernel<(V() & 1) != 0, (V() & 2) != 0>), grid,
                               dim3(PREP_THREADS), 0, s, (const int *)vis_in, (const int *)source,
                               (const int *)auto_source, channel_flags, (float2 *)vis, input_flags,
                               weights, items, runs_per_row, channels, in_baselines, baselines,
                               (long long)vis_in_stride, (long long)vis_stride,
                               (long long)input_flags_stride, (long long)weights_stride, scale,
                               weight_scale, (unsigned)lost_flag, aligned);
        });
    KSP_LAUNCH_CHECK();
    return 0;
}
