// average: flag-aware accumulation of visibilities over dumps and the finishing pass that
// sums groups of channels and divides by the weight (no reference counterpart: the
// reference's callers do this in their own code). rfi/host.py AveragerHost is the
// definition; both kernels reproduce it bit for bit, so every step below is one float32
// operation in the host's order (the translation unit is built with -ffp-contract=off and
// correctly rounded division, and the sums are written with __fmul_rn / __fadd_rn, which
// are never contracted).
//
//   accumulate, per sample:  f = flags | input_flags;  we = f ? w * 2^-64 : w;
//                            acc_vis += we * vis (re and im apart);  acc_weights += we;
//                            acc_flags |= f
//   finalise, per output:    re, im, w, fl = sum / OR over channel_factor rows, in order,
//                            from +0;  allbad = w < 2^-32: then re, im, w *= 2^64;
//                            vis = w > 0 ? (re / w, im / w) : 0;  flags = allbad ? fl : 0
//
// Layout. All arrays are [channels][stride] with baselines contiguous. A lane owns a run of
// AVG_RUN = 16 adjacent baselines of one row: 16 flag bytes (one 16-byte load), 128 bytes of
// visibilities (8 loads) and 64 bytes of weights (4). Runs are numbered row by row
// (run = row * runs_per_row + i) and dealt to the threads of a one-dimensional grid, so a
// narrow array still fills its wavefronts and the row count is not bound by the 65535 of the
// other grid dimensions. When every pointer and every row start is 16-byte aligned, a lane whose
// run lies wholly inside the row moves it with 16-byte loads and stores; the run at the end of
// a row, and every run of an unaligned call, goes element by element and touches only
// elements inside the row: padding is neither read nor written. (The run of run16.h, by hand:
// written on its helpers, with the arithmetic stated once, both kernels were slower on the
// 16-byte path, profiles/run16.md.)
//
// Traffic per sample: accumulate reads 8 (vis) + 1 (flags) + 4 (weights) and
// reads and writes 8 + 4 + 1 of accumulators: 39 bytes, 35 without weights, plus one byte for
// a FULL mask. finalise reads 13 and, with clear, writes 13, plus 13 / channel_factor out.
#include "launch.h"

#define AVG_THREADS 256
#define AVG_RUN 16

#define AVG_FLAGGED_SCALE 0x1p-64f
#define AVG_UNSCALE 0x1p64f
#define AVG_ALL_FLAGGED_BELOW 0x1p-32f

// One sample of the accumulation. `f` is the flag byte after the mask, in the low 8 bits.
template <bool HAS_W>
__device__ __forceinline__ void avg_add(float vre, float vim, float w, unsigned f, float &are,
                                        float &aim, float &aw)
{
    const float w1 = HAS_W ? w : 1.0f;
    const float we = f != 0 ? __fmul_rn(w1, AVG_FLAGGED_SCALE) : w1;
    are = __fadd_rn(are, __fmul_rn(we, vre));
    aim = __fadd_rn(aim, __fmul_rn(we, vim));
    aw = __fadd_rn(aw, we);
}

// MODE: 0 no input flags, 1 one byte per row, 2 one byte per sample.
template <bool HAS_W, int MODE>
__global__ __launch_bounds__(AVG_THREADS) void average_accumulate_kernel(
    const float2 *__restrict__ vis, const uint8_t *__restrict__ flags,
    const float *__restrict__ weights, const uint8_t *__restrict__ input_flags,
    float2 *__restrict__ acc_vis, float *__restrict__ acc_weights,
    uint8_t *__restrict__ acc_flags, long long runs, int runs_per_row, int baselines,
    long long vis_stride, long long flags_stride, long long weights_stride,
    long long input_flags_stride, long long acc_vis_stride, long long acc_weights_stride,
    long long acc_flags_stride, int aligned)
{
    const long long run = (long long)blockIdx.x * AVG_THREADS + threadIdx.x;
    if (run >= runs) return;
    const long long row = run / runs_per_row;
    const int col0 = (int)(run - row * runs_per_row) * AVG_RUN;
    const int valid = min(AVG_RUN, baselines - col0);  // >= 1

    const float2 *v = vis + row * vis_stride + col0;
    const uint8_t *fl = flags + row * flags_stride + col0;
    const float *w = HAS_W ? weights + row * weights_stride + col0 : nullptr;
    const uint8_t *in = MODE == 2 ? input_flags + row * input_flags_stride + col0 : nullptr;
    float2 *av = acc_vis + row * acc_vis_stride + col0;
    float *aw = acc_weights + row * acc_weights_stride + col0;
    uint8_t *af = acc_flags + row * acc_flags_stride + col0;
    // the row's mask byte in every byte of a word
    const unsigned row_mask = MODE == 1 ? input_flags[row] * 0x01010101u : 0u;

    if (aligned && valid == AVG_RUN) {
        uint4 f4 = *reinterpret_cast<const uint4 *>(fl);
        if (MODE == 2) {
            const uint4 m4 = *reinterpret_cast<const uint4 *>(in);
            f4 = make_uint4(f4.x | m4.x, f4.y | m4.y, f4.z | m4.z, f4.w | m4.w);
        }
        f4 = make_uint4(f4.x | row_mask, f4.y | row_mask, f4.z | row_mask, f4.w | row_mask);
        const unsigned fw[4] = {f4.x, f4.y, f4.z, f4.w};
        // four samples (one word of flags) at a time: 2 + 1 + 2 + 1 loads of 16 bytes
        float4 vv[4][2], aa[4][2], ww[4], wa[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            vv[q][0] = reinterpret_cast<const float4 *>(v)[2 * q];
            vv[q][1] = reinterpret_cast<const float4 *>(v)[2 * q + 1];
            aa[q][0] = reinterpret_cast<const float4 *>(av)[2 * q];
            aa[q][1] = reinterpret_cast<const float4 *>(av)[2 * q + 1];
            ww[q] = HAS_W ? reinterpret_cast<const float4 *>(w)[q] : make_float4(1, 1, 1, 1);
            wa[q] = reinterpret_cast<const float4 *>(aw)[q];
        }
        uint4 a4 = *reinterpret_cast<const uint4 *>(af);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            avg_add<HAS_W>(vv[q][0].x, vv[q][0].y, ww[q].x, fw[q] & 0xffu, aa[q][0].x, aa[q][0].y,
                           wa[q].x);
            avg_add<HAS_W>(vv[q][0].z, vv[q][0].w, ww[q].y, fw[q] & 0xff00u, aa[q][0].z,
                           aa[q][0].w, wa[q].y);
            avg_add<HAS_W>(vv[q][1].x, vv[q][1].y, ww[q].z, fw[q] & 0xff0000u, aa[q][1].x,
                           aa[q][1].y, wa[q].z);
            avg_add<HAS_W>(vv[q][1].z, vv[q][1].w, ww[q].w, fw[q] & 0xff000000u, aa[q][1].z,
                           aa[q][1].w, wa[q].w);
            reinterpret_cast<float4 *>(av)[2 * q] = aa[q][0];
            reinterpret_cast<float4 *>(av)[2 * q + 1] = aa[q][1];
            reinterpret_cast<float4 *>(aw)[q] = wa[q];
        }
        a4 = make_uint4(a4.x | f4.x, a4.y | f4.y, a4.z | f4.z, a4.w | f4.w);
        *reinterpret_cast<uint4 *>(af) = a4;
    } else {
        for (int i = 0; i < valid; i++) {
            unsigned f = fl[i] | (row_mask & 0xffu);
            if (MODE == 2) f |= in[i];
            float2 a = av[i];
            float sw = aw[i];
            const float2 z = v[i];
            avg_add<HAS_W>(z.x, z.y, HAS_W ? w[i] : 1.0f, f, a.x, a.y, sw);
            av[i] = a;
            aw[i] = sw;
            af[i] = (uint8_t)(af[i] | f);
        }
    }
}

// One output sample from its sums.
__device__ __forceinline__ void avg_finish(float re, float im, float w, unsigned fl, float2 &vis,
                                           float &weight, unsigned &flags)
{
    const bool allbad = w < AVG_ALL_FLAGGED_BELOW;
    if (allbad) {
        w = __fmul_rn(w, AVG_UNSCALE);
        re = __fmul_rn(re, AVG_UNSCALE);
        im = __fmul_rn(im, AVG_UNSCALE);
    }
    const bool some = w > 0.0f;
    vis.x = some ? __fdiv_rn(re, w) : 0.0f;
    vis.y = some ? __fdiv_rn(im, w) : 0.0f;
    weight = w;
    flags = allbad ? fl : 0u;
}

// A lane owns a run of 16 baselines of one OUTPUT row and walks the channel_factor rows of the
// accumulators that feed it in order, which makes the order of the sums the host's.
template <bool CLEAR>
__global__ __launch_bounds__(AVG_THREADS) void average_finalise_kernel(
    float2 *__restrict__ acc_vis, float *__restrict__ acc_weights, uint8_t *__restrict__ acc_flags,
    float2 *__restrict__ out_vis, float *__restrict__ out_weights, uint8_t *__restrict__ out_flags,
    long long runs, int runs_per_row, int baselines, int channel_factor, long long acc_vis_stride,
    long long acc_weights_stride, long long acc_flags_stride, long long out_vis_stride,
    long long out_weights_stride, long long out_flags_stride, int aligned)
{
    const long long run = (long long)blockIdx.x * AVG_THREADS + threadIdx.x;
    if (run >= runs) return;
    const long long row = run / runs_per_row;
    const int col0 = (int)(run - row * runs_per_row) * AVG_RUN;
    const int valid = min(AVG_RUN, baselines - col0);  // >= 1
    const long long row0 = row * channel_factor;

    float2 *av = acc_vis + row0 * acc_vis_stride + col0;
    float *aw = acc_weights + row0 * acc_weights_stride + col0;
    uint8_t *af = acc_flags + row0 * acc_flags_stride + col0;
    float2 *ov = out_vis + row * out_vis_stride + col0;
    float *ow = out_weights + row * out_weights_stride + col0;
    uint8_t *of = out_flags + row * out_flags_stride + col0;

    if (aligned && valid == AVG_RUN) {
        float4 sv[8], sw[4];  // sv[j]: samples 2 j and 2 j + 1 as re, im, re, im
        uint4 sf = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 8; j++) sv[j] = make_float4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) sw[j] = make_float4(0, 0, 0, 0);
        const float4 zero4 = make_float4(0, 0, 0, 0);
        for (int k = 0; k < channel_factor; k++) {
            float4 lv[8], lw[4];
#pragma unroll
            for (int j = 0; j < 8; j++) lv[j] = reinterpret_cast<const float4 *>(av)[j];
#pragma unroll
            for (int j = 0; j < 4; j++) lw[j] = reinterpret_cast<const float4 *>(aw)[j];
            const uint4 lf = *reinterpret_cast<const uint4 *>(af);
            if (CLEAR) {
#pragma unroll
                for (int j = 0; j < 8; j++) reinterpret_cast<float4 *>(av)[j] = zero4;
#pragma unroll
                for (int j = 0; j < 4; j++) reinterpret_cast<float4 *>(aw)[j] = zero4;
                *reinterpret_cast<uint4 *>(af) = make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                sv[j].x = __fadd_rn(sv[j].x, lv[j].x);
                sv[j].y = __fadd_rn(sv[j].y, lv[j].y);
                sv[j].z = __fadd_rn(sv[j].z, lv[j].z);
                sv[j].w = __fadd_rn(sv[j].w, lv[j].w);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                sw[j].x = __fadd_rn(sw[j].x, lw[j].x);
                sw[j].y = __fadd_rn(sw[j].y, lw[j].y);
                sw[j].z = __fadd_rn(sw[j].z, lw[j].z);
                sw[j].w = __fadd_rn(sw[j].w, lw[j].w);
            }
            sf = make_uint4(sf.x | lf.x, sf.y | lf.y, sf.z | lf.z, sf.w | lf.w);
            av += acc_vis_stride;
            aw += acc_weights_stride;
            af += acc_flags_stride;
        }
        const unsigned fw[4] = {sf.x, sf.y, sf.z, sf.w};
        unsigned outf[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float wq[4] = {sw[q].x, sw[q].y, sw[q].z, sw[q].w};
            float wo[4];
            outf[q] = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float4 s = sv[2 * q + h];
                float2 z0, z1;
                unsigned f0, f1;
                avg_finish(s.x, s.y, wq[2 * h], (fw[q] >> (16 * h)) & 0xffu, z0, wo[2 * h], f0);
                avg_finish(s.z, s.w, wq[2 * h + 1], (fw[q] >> (16 * h + 8)) & 0xffu, z1,
                           wo[2 * h + 1], f1);
                outf[q] |= (f0 << (16 * h)) | (f1 << (16 * h + 8));
                reinterpret_cast<float4 *>(ov)[2 * q + h] = make_float4(z0.x, z0.y, z1.x, z1.y);
            }
            reinterpret_cast<float4 *>(ow)[q] = make_float4(wo[0], wo[1], wo[2], wo[3]);
        }
        *reinterpret_cast<uint4 *>(of) = make_uint4(outf[0], outf[1], outf[2], outf[3]);
    } else {
        for (int i = 0; i < valid; i++) {
            float re = 0.0f, im = 0.0f, w = 0.0f;
            unsigned f = 0;
            for (int k = 0; k < channel_factor; k++) {
                float2 *pv = av + k * acc_vis_stride + i;
                float *pw = aw + k * acc_weights_stride + i;
                uint8_t *pf = af + k * acc_flags_stride + i;
                const float2 z = *pv;
                re = __fadd_rn(re, z.x);
                im = __fadd_rn(im, z.y);
                w = __fadd_rn(w, *pw);
                f |= *pf;
                if (CLEAR) {
                    *pv = make_float2(0.0f, 0.0f);
                    *pw = 0.0f;
                    *pf = 0;
                }
            }
            float2 z;
            float wo;
            unsigned fo;
            avg_finish(re, im, w, f, z, wo, fo);
            ov[i] = z;
            ow[i] = wo;
            of[i] = (uint8_t)fo;
        }
    }
}

extern "C" int ksp_average_accumulate(int device, void *stream, const void *vis,
                                      const uint8_t *flags, const float *weights,
                                      const uint8_t *input_flags, int input_flags_mode,
                                      void *acc_vis, float *acc_weights, uint8_t *acc_flags,
                                      int channels, int baselines, int vis_stride,
                                      int flags_stride, int weights_stride,
                                      int input_flags_stride, int acc_vis_stride,
                                      int acc_weights_stride, int acc_flags_stride)
{
    // (input_flags has a row stride only as one byte per sample, and checks of its own)
    const ksp_planes planes = {
        {"vis", vis, vis_stride, 8},
        {"flags", flags, flags_stride, 1},
        {"weights", weights, weights_stride, 4, true},
        {"input_flags", input_flags_mode == 2 ? input_flags : nullptr, input_flags_stride, 1, true},
        {"acc_vis", acc_vis, acc_vis_stride, 8},
        {"acc_weights", acc_weights, acc_weights_stride, 4},
        {"acc_flags", acc_flags, acc_flags_stride, 1}};
    KSP_TRY(ksp_planes_given(planes));
    KSP_REQUIRE(input_flags_mode >= 0 && input_flags_mode <= 2,
                "input_flags_mode must be 0 (none), 1 (per channel) or 2 (per sample)");
    KSP_REQUIRE(input_flags_mode == 0 || input_flags != nullptr,
                "input_flags is NULL but input_flags_mode is not 0");
    KSP_REQUIRE(input_flags_mode != 0 || input_flags == nullptr,
                "input_flags given but input_flags_mode is 0");
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_TRY(ksp_planes_hold(planes, baselines, "baselines"));
    ksp_run_grid g;
    KSP_TRY(ksp_make_run_grid(channels, baselines, AVG_RUN, AVG_THREADS, g));
    const int aligned = ksp_planes_aligned(planes);

    KSP_CHECK(hipSetDevice(device));
    ksp_dispatch_bool(weights != nullptr, [&](auto HAS_W) {
        // (input_flags_mode is 0 .. 2 here)
        ksp_dispatch_exact<0, 1, 2>(input_flags_mode, [&](auto MODE) {
            hipLaunchKernelGGL(
                (average_accumulate_kernel<decltype(HAS_W)::value, MODE()>),
                dim3((unsigned)g.groups), dim3(AVG_THREADS), 0, (hipStream_t)stream,
                (const float2 *)vis, flags, weights, input_flags, (float2 *)acc_vis, acc_weights,
                acc_flags, g.runs, g.runs_per_row, baselines, (long long)vis_stride,
                (long long)flags_stride, (long long)weights_stride,
                (long long)input_flags_stride, (long long)acc_vis_stride,
                (long long)acc_weights_stride, (long long)acc_flags_stride, aligned);
        });
    });
    KSP_LAUNCH_CHECK();
    return 0;
}

extern "C" int ksp_average_finalise(int device, void *stream, void *acc_vis, float *acc_weights,
                                    uint8_t *acc_flags, void *out_vis, float *out_weights,
                                    uint8_t *out_flags, int channels, int baselines,
                                    int channel_factor, int clear, int acc_vis_stride,
                                    int acc_weights_stride, int acc_flags_stride,
                                    int out_vis_stride, int out_weights_stride,
                                    int out_flags_stride)
{
    const ksp_planes planes = {{"acc_vis", acc_vis, acc_vis_stride, 8},
                               {"acc_weights", acc_weights, acc_weights_stride, 4},
                               {"acc_flags", acc_flags, acc_flags_stride, 1},
                               {"out_vis", out_vis, out_vis_stride, 8},
                               {"out_weights", out_weights, out_weights_stride, 4},
                               {"out_flags", out_flags, out_flags_stride, 1}};
    KSP_TRY(ksp_planes_given(planes));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(channel_factor >= 1, "channel_factor must be at least 1");
    KSP_REQUIRE(channels % channel_factor == 0, "channel_factor does not divide channels");
    KSP_TRY(ksp_planes_hold(planes, baselines, "baselines"));
    ksp_run_grid g;
    KSP_TRY(ksp_make_run_grid(channels / channel_factor, baselines, AVG_RUN, AVG_THREADS, g));
    const int aligned = ksp_planes_aligned(planes);

    KSP_CHECK(hipSetDevice(device));
    ksp_dispatch_bool(clear != 0, [&](auto CLEAR) {
        hipLaunchKernelGGL(average_finalise_kernel<CLEAR()>, dim3((unsigned)g.groups),
                           dim3(AVG_THREADS), 0, (hipStream_t)stream, (float2 *)acc_vis,
                           acc_weights, acc_flags, (float2 *)out_vis, out_weights, out_flags,
                           g.runs, g.runs_per_row, baselines, channel_factor,
                           (long long)acc_vis_stride, (long long)acc_weights_stride,
                           (long long)acc_flags_stride, (long long)out_vis_stride,
                           (long long)out_weights_stride, (long long)out_flags_stride, aligned);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}

