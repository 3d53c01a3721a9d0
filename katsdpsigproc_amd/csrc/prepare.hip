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
//     input_flags = cf | baseline_flags[j] | (lost ? lost_flag : 0)
//       cf = channel_flags[c], or with mask_index (classes rows of channel_flags):
//       k = mask_index[j];  cf = k < classes ? channel_flags[k][c] : 0
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
// Flags per baseline. mask_index and baseline_flags are one byte per output baseline, so a
// lane keeps its run's 16 of each as four packed words (one 16-byte load each on the 16-byte
// path, byte loads on the other) for all rows of its item, beside the source entries. The
// classes' bytes of a row (channel_flags[k][row], k < classes <= 8) are the same for every
// lane of the row: a lane loads them once per row into a pair of words, byte k for class k
// and zero above `classes`, and picks the bytes of four samples at once with one v_perm_b32.
// Its selectors are made once per run from the mask indices: the index itself below 8, and
// 12, the selector of a zero byte, for everything else. So every uint8 in mask_index has a
// result and none reaches an address. The element-wise path has no run to share a row's
// words with: it loads the one byte it needs, from class 0 when the index is outside, and
// drops it then.
//
// Traffic per sample: 8 bytes gathered, 8 + 1 written, 4 more with weights; the flags per
// baseline are 2 bytes per 16 samples and group of rows.
#include <limits.h>

#include "launch.h"

#define PREP_THREADS 256
#define PREP_RUN 16
#define PREP_ROWS(has_w) ((has_w) ? 4 : 2)
#define PREP_MAX_CLASSES 8

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

// channel_flags[k][row] of the classes k < `classes` (1 .. 8) as byte k of the eight bytes of
// (lo, hi); the bytes at and above `classes` are zero. Eight loads whatever `classes` is,
// those of the classes that are not there from class 0.
__device__ __forceinline__ void prep_class_words(const uint8_t *__restrict__ channel_flags,
                                                 long long stride, long long row, int classes,
                                                 unsigned &lo, unsigned &hi)
{
    unsigned w[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < PREP_MAX_CLASSES; k++) {
        const bool there = k < classes;
        const unsigned b = channel_flags[(there ? k : 0) * stride + row];
        w[k / 4] |= (there ? b : 0u) << (8 * (k % 4));
    }
    lo = w[0];
    hi = w[1];
}

// Four mask indices (the bytes of `index`) as the selectors of v_perm_b32 on such a pair: 0 .. 7
// pick that byte of (lo, hi), 12 gives a zero byte and stands for every index of 8 or more.
__device__ __forceinline__ unsigned prep_class_selectors(unsigned index)
{
    unsigned sel = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned m = (index >> (8 * k)) & 0xffu;
        sel |= (m < (unsigned)PREP_MAX_CLASSES ? m : 12u) << (8 * k);
    }
    return sel;
}

// The instances with weights take 191 registers (two waves per SIMD): 48 indices, the 64 words
// of a row's gathers and the 64-bit addresses of the loads in flight. Held to three waves they
// were slower (profiles/prepare.md), held to four they spill: no occupancy bound.
// HAS_MI (classes of channel masks by mask_index; needs HAS_CF) and HAS_BF (baseline_flags)
// are off in the four instances of ksp_prepare, which then do not touch the last four
// arguments.
template <bool HAS_CF, bool HAS_W, bool HAS_MI, bool HAS_BF>
__global__ __launch_bounds__(PREP_THREADS) void prepare_kernel(
    const int *__restrict__ vis_in, const int *__restrict__ source,
    const int *__restrict__ auto_source, const uint8_t *__restrict__ channel_flags,
    float2 *__restrict__ vis, uint8_t *__restrict__ input_flags, float *__restrict__ weights,
    long long items, int runs_per_row, int channels, int in_baselines, int baselines,
    long long vis_in_stride, long long vis_stride, long long input_flags_stride,
    long long weights_stride, float scale, float weight_scale, unsigned lost_flag, int aligned,
    const uint8_t *__restrict__ mask_index, const uint8_t *__restrict__ baseline_flags,
    long long channel_flags_stride, int classes)
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
        // and its mask indices (as selectors) and baseline flags, four bytes to a word
        uint4 mi = make_uint4(0, 0, 0, 0), bf = make_uint4(0, 0, 0, 0);
        if (HAS_MI) mi = *reinterpret_cast<const uint4 *>(mask_index + col0);
        if (HAS_BF) bf = *reinterpret_cast<const uint4 *>(baseline_flags + col0);
        const unsigned sel[4] = {prep_class_selectors(mi.x), prep_class_selectors(mi.y),
                                 prep_class_selectors(mi.z), prep_class_selectors(mi.w)};
        const unsigned bfw[4] = {bf.x, bf.y, bf.z, bf.w};
        for (int r = 0; r < rows; r++) {
            const long long row = row0 + r;
            const int *in = vis_in + 2 * row * vis_in_stride;
            float2 *v = vis + row * vis_stride + col0;
            uint8_t *fl = input_flags + row * input_flags_stride + col0;
            const unsigned cf = HAS_CF && !HAS_MI ? channel_flags[row] : 0u;
            unsigned cw_lo = 0, cw_hi = 0;
            if (HAS_MI)
                prep_class_words(channel_flags, channel_flags_stride, row, classes, cw_lo, cw_hi);
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
                if (HAS_BF) fw[q] |= bfw[q];
                if (HAS_MI) fw[q] |= __builtin_amdgcn_perm(cw_hi, cw_lo, sel[q]);
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
            // the class as an index that is inside, like source: class 0 when it is not
            const unsigned m = HAS_MI ? mask_index[col0 + i] : 0u;
            const bool ok_m = m < (unsigned)classes;
            const long long cf0 = HAS_MI ? (ok_m ? m : 0u) * channel_flags_stride : 0;
            const unsigned bfi = HAS_BF ? baseline_flags[col0 + i] : 0u;
            for (int r = 0; r < rows; r++) {
                const long long row = row0 + r;
                const int *in = vis_in + 2 * row * vis_in_stride;
                const int re = in[2 * (long long)si], im = in[2 * (long long)si + 1];
                const bool lost = !ok || re == INT_MIN;
                float2 z;
                z.x = lost ? 0.0f : __fmul_rn((float)re, scale);
                z.y = lost ? 0.0f : __fmul_rn((float)im, scale);
                vis[row * vis_stride + col0 + i] = z;
                unsigned cf = HAS_CF ? channel_flags[cf0 + row] : 0u;
                if (HAS_MI) cf = ok_m ? cf : 0u;
                input_flags[row * input_flags_stride + col0 + i] =
                    (uint8_t)(cf | bfi | (lost ? lost_flag : 0u));
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

extern "C" int ksp_prepare_flags(int device, void *stream, const int32_t *vis_in,
                                 const int32_t *source, const int32_t *auto_source,
                                 const uint8_t *channel_flags, const uint8_t *mask_index,
                                 const uint8_t *baseline_flags, void *vis, uint8_t *input_flags,
                                 float *weights, int channels, int in_baselines, int baselines,
                                 int mask_classes, int vis_in_stride, int channel_flags_stride,
                                 int vis_stride, int input_flags_stride, int weights_stride,
                                 float scale, float weight_scale, int lost_flag)
{
    const ksp_plane raw = {"vis_in", vis_in, vis_in_stride, 4};
    const ksp_planes tables = {{"source", source, 0, 4},
                               {"auto_source", auto_source, 0, 4, true},
                               {"mask_index", mask_index, 0, 1, true},
                               {"baseline_flags", baseline_flags, 0, 1, true}};
    const ksp_planes out = {{"vis", vis, vis_stride, 8},
                            {"input_flags", input_flags, input_flags_stride, 1},
                            {"weights", weights, weights_stride, 4, true}};
    // (the row stride of channel_flags is looked at only with classes of masks)
    const ksp_plane masks = {"channel_flags", mask_classes != 0 ? channel_flags : nullptr,
                             channel_flags_stride, 1, true};
    KSP_TRY(ksp_planes_given({raw}));
    KSP_TRY(ksp_planes_given(tables));
    KSP_TRY(ksp_planes_given(out));
    KSP_REQUIRE((auto_source == nullptr) == (weights == nullptr),
                "auto_source and weights must both be given or both be NULL");
    KSP_REQUIRE(mask_classes >= 0 && mask_classes <= PREP_MAX_CLASSES,
                "mask_classes must be 0..8");
    KSP_REQUIRE((mask_index == nullptr) == (mask_classes == 0),
                "mask_index must be given exactly when mask_classes is not 0");
    KSP_REQUIRE(mask_classes == 0 || channel_flags != nullptr,
                "mask_classes of 1 or more need channel_flags");
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(in_baselines >= 1, "in_baselines must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_TRY(ksp_planes_hold({raw}, in_baselines, "in_baselines"));
    KSP_TRY(ksp_planes_hold({masks}, channels, "channels"));
    KSP_TRY(ksp_planes_hold(out, baselines, "baselines"));
    KSP_REQUIRE(prep_positive(scale), "scale must be finite and positive");
    KSP_REQUIRE(weights == nullptr || prep_positive(weight_scale),
                "weight_scale must be finite and positive");
    KSP_REQUIRE(lost_flag >= 1 && lost_flag <= 255, "lost_flag must be 1..255");
    // an item is a run of PREP_ROWS rows
    const int rows_per_item = PREP_ROWS(weights != nullptr);
    ksp_run_grid g;
    KSP_TRY(ksp_make_run_grid(((long long)channels + rows_per_item - 1) / rows_per_item,
                              baselines, PREP_RUN, PREP_THREADS, g));
    // (vis_in is read in pairs of words, the tables and the outputs 16 bytes at a time)
    const int aligned =
        (uintptr_t)vis_in % 8 == 0 && ksp_planes_aligned(tables) && ksp_planes_aligned(out);

    KSP_CHECK(hipSetDevice(device));
    // bit 0: channel mask, 1: weights, 2: classes of masks (only with bit 0), 3: baseline flags
    const int variant = (channel_flags != nullptr ? 1 : 0) + (weights != nullptr ? 2 : 0) +
                        (mask_index != nullptr ? 4 : 0) + (baseline_flags != nullptr ? 8 : 0);
    ksp_dispatch_exact<0, 1, 2, 3, 5, 7, 8, 9, 10, 11, 13, 15>(variant, [&](auto V) {
        hipLaunchKernelGGL(
            (prepare_kernel<(V() & 1) != 0, (V() & 2) != 0, (V() & 4) != 0, (V() & 8) != 0>),
            dim3((unsigned)g.groups), dim3(PREP_THREADS), 0, (hipStream_t)stream,
            (const int *)vis_in, (const int *)source, (const int *)auto_source, channel_flags,
            (float2 *)vis, input_flags, weights, g.runs, g.runs_per_row, channels, in_baselines,
            baselines, (long long)vis_in_stride, (long long)vis_stride,
            (long long)input_flags_stride, (long long)weights_stride, scale, weight_scale,
            (unsigned)lost_flag, aligned, mask_index, baseline_flags,
            (long long)channel_flags_stride, mask_classes);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}

// The four instances without classes and baseline flags, with the checks and results it had
// before ksp_prepare_flags.
extern "C" int ksp_prepare(int device, void *stream, const int32_t *vis_in, const int32_t *source,
                           const int32_t *auto_source, const uint8_t *channel_flags, void *vis,
                           uint8_t *input_flags, float *weights, int channels, int in_baselines,
                           int baselines, int vis_in_stride, int vis_stride,
                           int input_flags_stride, int weights_stride, float scale,
                           float weight_scale, int lost_flag)
{
    return ksp_prepare_flags(device, stream, vis_in, source, auto_source, channel_flags, nullptr,
                             nullptr, vis, input_flags, weights, channels, in_baselines, baselines,
                             0, vis_in_stride, 0, vis_stride, input_flags_stride, weights_stride,
                             scale, weight_scale, lost_flag);
}
