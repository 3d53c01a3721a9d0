// apply_gains: per-input gain corrections applied to visibilities, weights and flags, in one
// launch (no reference counterpart). rfi/host.py ApplyGainsHost is the definition; the kernel
// reproduces it bit for bit, so every float step below is one float32 operation (the
// translation unit is built with -ffp-contract=off and correctly rounded division, and the
// steps are written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, which are never
// contracted).
//
//   per channel c and baseline j, with (a, b) = inputs[j]:
//     inr = 0 <= a < n_inputs and 0 <= b < n_inputs       (an index outside forms no address)
//     ga = gains[c][a], gb = gains[c][b]
//     cr = ga.re * gb.re + ga.im * gb.im;  ci = ga.im * gb.re - ga.re * gb.im   (ga conj(gb))
//     ok = inr and cr, ci are not NaN;     p = cr * cr + ci * ci
//     out_vis     = ok ? (v.re * cr - v.im * ci, v.re * ci + v.im * cr) : v
//     out_weights = ok and p > 0 ? w / p : 0
//     out_flags   = flags | (ok ? 0 : flag_value)
//
// Layout. The six sample arrays are [channels][stride] with baselines contiguous, and a lane
// owns a run of KSP_RUN = 16 adjacent baselines (run16.h). The lane keeps the 32 indices of its
// run in registers for as long as it lives, so `inputs` is read once per lane, not once per
// sample. The gains are gathered through LDS: a workgroup copies whole rows of `gains` into
// AG_LDS_GAINS = 4096 slots of 8 bytes (32 KiB), as many rows as fit (ag_stage_rows, which
// depends on n_inputs alone), and every lane then picks its 32 gains per row with 8-byte LDS
// reads. A sample costs 16 bytes of LDS reads.
//
// Geometry (tile_grid.h). A workgroup of 256 threads owns a tile of `tile_runs` runs (1 .. 256,
// so a tile is at most 4096 baselines wide) and a chunk of `chunk` rows, about AG_TARGET_GROUPS
// workgroups to a launch: thread t owns run t % tile_runs of the tile and, of each stage, the
// rows t / tile_runs, t / tile_runs + 256 / tile_runs, ... A workgroup walks its chunk in stages
// of at most ag_stage_rows rows, two barriers per stage. Row bases are 64-bit.
//
// In place. A lane loads the vis, weights and flags of a run before it stores any of them, and
// no other lane touches that run, so an output may be its input (same pointer, same stride). The
// sample pointers are therefore not __restrict__.
//
// The 16-byte accesses apply when every sample array given and each of its row starts is a
// multiple of 16 bytes (one flag for the six), and to `inputs` when it is (another).
//
// Traffic per sample: 8 + 4 + 1 bytes read and as many written, 26 in all (24, 18 and 16
// without flags, weights or both); per lane 128 bytes of indices; per workgroup and stage the
// rows of gains it stages, which come from L2 for all but the first workgroup to ask.
#include "cal_math.h"
#include "launch.h"
#include "run16.h"
#include "tile_grid.h"

#define AG_THREADS 256
#define AG_LDS_GAINS 4096       // gains a stage holds (8 bytes each)
#define AG_MAX_INPUTS 4096      // so one row always fits
#define AG_STAGE_ROWS_MAX 256   // no stage is taller (one row per thread)
#ifndef AG_TARGET_GROUPS  // (an experiment's -D, KSP_EXTRA_HIPCC_FLAGS)
#define AG_TARGET_GROUPS 1024  // (512 .. 4096 timed: profiles/apply_gains.md)
#endif
#define AG_ALIGNED_DATA 1
#define AG_ALIGNED_INPUTS 2

// Rows of gains per stage (tests/test_gpu_apply_gains.py has the same formula)
static int ag_stage_rows(int n_inputs)
{
    const int fit = AG_LDS_GAINS / n_inputs;
    return fit < AG_STAGE_ROWS_MAX ? fit : AG_STAGE_ROWS_MAX;
}

template <bool HAS_W, bool HAS_F>
__global__ __launch_bounds__(AG_THREADS) void apply_gains_kernel(
    const float2 *vis, const float *weights, const uint8_t *flags,
    const float2 *__restrict__ gains, const int *__restrict__ inputs, float2 *out_vis,
    float *out_weights, uint8_t *out_flags, int channels, int baselines, int n_inputs, int tiles,
    int tile_shift, int chunk, int stage_rows, long long vis_stride, long long weights_stride,
    long long flags_stride, long long gains_stride, long long out_vis_stride,
    long long out_weights_stride, long long out_flags_stride, unsigned flag_value, int aligned)
{
    __shared__ float2 staged[AG_LDS_GAINS];
    const bool wide = aligned & AG_ALIGNED_DATA;
    const int tid = threadIdx.x;
    const ksp_tile_place at =
        ksp_tile_locate(AG_THREADS, tiles, tile_shift, chunk, channels, baselines);
    const long long row_begin = at.row_begin, row_end = at.row_end, col0 = at.col0;
    const int slot = at.slot, slots = at.slots;
    const int valid = at.valid;  // (0: the lane only helps to stage)

    // The lane's indices, once. Those outside 0 .. n_inputs - 1 are replaced by 0 and remembered.
    // (element by element as int32, which is all the alignment an unaligned `inputs` promises)
    int2 idx[KSP_RUN];
    const int *own = inputs + 2 * col0;
    if ((aligned & AG_ALIGNED_INPUTS) && valid >= KSP_RUN) {
        ksp_run_load(reinterpret_cast<const int2 *>(own), valid, true, idx, make_int2(-1, -1));
    } else {
#pragma unroll
        for (int i = 0; i < KSP_RUN; i++)
            idx[i] = i < valid ? make_int2(own[2 * i], own[2 * i + 1]) : make_int2(-1, -1);
    }
    unsigned inr = 0;
#pragma unroll
    for (int i = 0; i < KSP_RUN; i++) {
        const bool in = (unsigned)idx[i].x < (unsigned)n_inputs &&
                        (unsigned)idx[i].y < (unsigned)n_inputs;
        inr |= (unsigned)in << i;
        if (!in) idx[i] = make_int2(0, 0);
    }

    // Staging walks the flat index of (row of the stage, input) in steps of the workgroup
    const int stage_r0 = tid / n_inputs, stage_c0 = tid - stage_r0 * n_inputs;
    const int stage_dr = AG_THREADS / n_inputs, stage_dc = AG_THREADS - stage_dr * n_inputs;

    for (long long s = row_begin; s < row_end; s += stage_rows) {
        const int n = (int)min((long long)stage_rows, row_end - s);  // n * n_inputs <= AG_LDS_GAINS
        for (int r = stage_r0, c = stage_c0, e = tid; r < n; e += AG_THREADS) {
            staged[e] = gains[(s + r) * gains_stride + c];
            r += stage_dr;
            c += stage_dc;
            if (c >= n_inputs) {
                c -= n_inputs;
                r++;
            }
        }
        __syncthreads();
        if (valid > 0) {
            for (int r = slot; r < n; r += slots) {
                const long long row = s + r;
                const float2 *g = staged + r * n_inputs;
                float2 v[KSP_RUN];
                float w[KSP_RUN];
                ksp_run_bytes f = {0, 0, 0, 0};
                ksp_run_load(vis + row * vis_stride + col0, valid, wide, v, make_float2(0, 0));
                if (HAS_W) ksp_run_load(weights + row * weights_stride + col0, valid, wide, w, 0.0f);
                if (HAS_F) f = ksp_run_load_bytes(flags + row * flags_stride + col0, valid, wide);
                unsigned bad = 0;
#pragma unroll
                for (int i = 0; i < KSP_RUN; i++) {
                    const float2 ga = g[idx[i].x], gb = g[idx[i].y];
                    // (ksp_cmul_conj(ga, gb) and ksp_cmul(v[i], c) written out: through the
                    // helpers the compiler allots other registers, 92 .. 192 to 102 .. 163)
                    const float cr = __fadd_rn(__fmul_rn(ga.x, gb.x), __fmul_rn(ga.y, gb.y));
                    const float ci = __fsub_rn(__fmul_rn(ga.y, gb.x), __fmul_rn(ga.x, gb.y));
                    const bool ok = ((inr >> i) & 1u) && !__builtin_isnan(cr) && !__builtin_isnan(ci);
                    const float p = ksp_norm2(make_float2(cr, ci));
                    const float re = __fsub_rn(__fmul_rn(v[i].x, cr), __fmul_rn(v[i].y, ci));
                    const float im = __fadd_rn(__fmul_rn(v[i].x, ci), __fmul_rn(v[i].y, cr));
                    v[i].x = ok ? re : v[i].x;
                    v[i].y = ok ? im : v[i].y;
                    if (HAS_W) w[i] = ok && p > 0.0f ? __fdiv_rn(w[i], p) : 0.0f;
                    bad |= (unsigned)!ok << i;
                }
                ksp_run_store(out_vis + row * out_vis_stride + col0, valid, wide, v);
                if (HAS_W)
                    ksp_run_store(out_weights + row * out_weights_stride + col0, valid, wide, w);
                if (HAS_F) {
                    ksp_flag_spread(f, bad, flag_value);
                    ksp_run_store_bytes(out_flags + row * out_flags_stride + col0, valid, wide, f);
                }
            }
        }
        __syncthreads();
    }
}

extern "C" int ksp_apply_gains(int device, void *stream, const void *vis, const float *weights,
                               const uint8_t *flags, const void *gains, const int32_t *inputs,
                               void *out_vis, float *out_weights, uint8_t *out_flags,
                               int channels, int baselines, int n_inputs, int vis_stride,
                               int weights_stride, int flags_stride, int gains_stride,
                               int out_vis_stride, int out_weights_stride, int out_flags_stride,
                               int flag_value)
{
    const ksp_plane in = {"vis", vis, vis_stride, 8}, out = {"out_vis", out_vis, out_vis_stride, 8};
    const ksp_plane table = {"gains", gains, gains_stride, 8};
    const ksp_planes pairs = {{"weights", weights, weights_stride, 4, true},
                              {"out_weights", out_weights, out_weights_stride, 4, true},
                              {"flags", flags, flags_stride, 1, true},
                              {"out_flags", out_flags, out_flags_stride, 1, true}};
    KSP_TRY(ksp_planes_given({in, table, {"inputs", inputs, 0, 4}, out}));
    KSP_TRY(ksp_pairs_given_together(pairs));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_inputs >= 1 && n_inputs <= AG_MAX_INPUTS, "n_inputs must be 1..4096");
    KSP_REQUIRE(flag_value >= 1 && flag_value <= 255, "flag_value must be 1..255");
    KSP_TRY(ksp_planes_hold({in, out}, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold({table}, n_inputs, "n_inputs"));
    KSP_TRY(ksp_planes_hold(pairs, baselines, "baselines"));
    KSP_TRY(ksp_pairs_same_or_apart({in, out}, channels, baselines));
    KSP_TRY(ksp_pairs_same_or_apart(pairs, channels, baselines));
    const ksp_tile_geometry geom =
        ksp_make_tile_geometry(channels, baselines, AG_THREADS, AG_THREADS, AG_TARGET_GROUPS);
    KSP_REQUIRE(geom.groups <= 0x7fffffffll, "array too large for one launch");
    // (the rows of gains are read element by element; inputs has a flag of its own)
    const int aligned =
        (ksp_planes_aligned({in, out}) && ksp_planes_aligned(pairs) ? AG_ALIGNED_DATA : 0) |
        ((uintptr_t)inputs % 16 == 0 ? AG_ALIGNED_INPUTS : 0);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int variant = (weights != nullptr ? 1 : 0) | (flags != nullptr ? 2 : 0);
    ksp_dispatch_exact<0, 1, 2, 3>(variant, [&](auto V) {
        hipLaunchKernelGGL((apply_gains_kernel<(V() & 1) != 0, (V() & 2) != 0>),
                           dim3((unsigned)geom.groups), dim3(AG_THREADS), 0, s, (const float2 *)vis,
                           weights, flags, (const float2 *)gains, (const int *)inputs,
                           (float2 *)out_vis, out_weights, out_flags, channels, baselines, n_inputs,
                           geom.tiles, geom.tile_shift, geom.chunk, ag_stage_rows(n_inputs),
                           (long long)vis_stride, (long long)weights_stride,
                           (long long)flags_stride, (long long)gains_stride,
                           (long long)out_vis_stride, (long long)out_weights_stride,
                           (long long)out_flags_stride, (unsigned)flag_value, aligned);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
