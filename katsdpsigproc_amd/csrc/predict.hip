// predict: model visibilities of point sources, and optionally the data divided by them, in one
// launch (no reference counterpart). rfi/host.py PredictHost is the definition; the kernel
// reproduces it bit for bit, so every float64 step of the model and every float32 step of the
// division is one operation, rounded once (the translation unit is built with
// -ffp-contract=off and correctly rounded division, and the steps are written with __dmul_rn /
// __dadd_rn / __dsub_rn and __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn).
//
//   per channel c, baseline j and source s = 0 .. n_sources - 1, in float64:
//     x  = freqs[c] * delays[s][j]                 turns
//     (co, si) = cos_sin(x)                        (cal_math.h: ksp_cos_sin_turns, the series)
//     re += flux[c][s] * co;  im -= flux[c][s] * si           from +0, s ascending
//   M = (float32(re), float32(im)) = model[c][j]; then, with vis, in float32:
//     d  = M.re * M.re + M.im * M.im;  ok = 0 < d < inf
//     out_vis     = ok ? ((v.re*M.re + v.im*M.im) / d, (v.im*M.re - v.re*M.im) / d) : v
//     out_weights = ok ? w * d : 0
//     out_flags   = flags | (ok ? 0 : flag_value)
//
// Layout. The sample arrays are [channels][stride] with baselines contiguous, and a lane owns a
// run of KSP_RUN = 16 adjacent baselines of one row (run16.h), with the 32 float64 accumulators
// of the run in registers. A workgroup of 256 threads owns a tile of `tile_runs` runs (a power
// of two, 1 .. PR_TILE_RUNS = 16: the narrowest that holds a row, so a tile is at most 256
// baselines wide) and a chunk of `chunk` rows; thread t owns run t % tile_runs of the tile and,
// of every batch of 256 / tile_runs rows, row t / tile_runs (tile_grid.h).
//
// The delays of the tile are staged in LDS, PR_BLOCK = 16 sources at a time (32 KiB), element
// i of run r of source s at word s * 256 + i * 16 + r whatever the tile's width: the lanes of
// adjacent runs read adjacent 8-byte words, the lanes that share a run read the same word, and
// the 16 offsets of a lane are immediates. With up to 16 sources the tile is staged once per
// workgroup; with more, the blocks are staged in turn for every batch of rows, because the
// accumulators of a row live through all of them (two barriers per block; 0.5 bytes from L2
// per sample and source). freqs[c] and flux[c][s] are loaded once per row and per row and
// source. A (sample, source) pair costs one 8-byte LDS read and PR_FLOPS_PER_PAIR float64
// instructions.
//
// In place. A lane loads the vis, weights and flags of a run before it stores any of them, and
// no other lane touches that run, so an output may be its input (same pointer, same stride). The
// sample pointers are therefore not __restrict__. model overlaps nothing.
//
// The 16-byte accesses apply when every sample array given (model included) and each of its row
// starts is a multiple of 16 bytes. freqs, delays and flux are read element by element.
//
// Traffic per sample: 8 bytes written for the model; 8 + 4 + 1 read and as many written for
// the division (24, 18, 16 without flags, weights or both); per workgroup the delays of its
// tile; per row of a lane 8 bytes of freqs and 4 bytes of flux per source, from L2.
#include <cmath>

#include "cal_math.h"
#include "launch.h"
#include "run16.h"
#include "tile_grid.h"

#define PR_THREADS 256
#define PR_TILE_RUNS 16    // runs of a tile at most
#define PR_BLOCK 16        // sources a stage holds
#define PR_MAX_SOURCES 64
#ifndef PR_TARGET_GROUPS  // (an experiment's -D, KSP_EXTRA_HIPCC_FLAGS)
#define PR_TARGET_GROUPS 4096
#endif
// float64 instructions per (sample, source) as written below and in ksp_cos_sin_turns: x (1),
// r (2), q (2), y (2), z and z2 (2), sn (11), cs (12), the two products and the two sums (4)
#define PR_FLOPS_PER_PAIR 36

#define PR_MODEL 1
#define PR_DIVIDE 2
#define PR_WEIGHTS 4
#define PR_FLAGS 8

template <int VARIANT>
__global__ __launch_bounds__(PR_THREADS) void predict_kernel(
    const double *__restrict__ freqs, const double *__restrict__ delays,
    const float *__restrict__ flux, float2 *__restrict__ model, const float2 *vis,
    const float *weights, const uint8_t *flags, float2 *out_vis, float *out_weights,
    uint8_t *out_flags, int channels, int baselines, int n_sources, int tiles, int tile_shift,
    int chunk, long long delays_stride, long long flux_stride, long long model_stride,
    long long vis_stride, long long weights_stride, long long flags_stride,
    long long out_vis_stride, long long out_weights_stride, long long out_flags_stride,
    unsigned flag_value, bool wide)
{
    constexpr bool HAS_M = VARIANT & PR_MODEL, HAS_V = VARIANT & PR_DIVIDE;
    constexpr bool HAS_W = VARIANT & PR_WEIGHTS, HAS_F = VARIANT & PR_FLAGS;
    __shared__ double staged[PR_BLOCK * PR_TILE_RUNS * KSP_RUN];
    const int tid = threadIdx.x;
    const ksp_tile_place at =
        ksp_tile_locate(PR_THREADS, tiles, tile_shift, chunk, channels, baselines);
    const long long row_begin = at.row_begin, row_end = at.row_end;
    const long long tile_col0 = at.tile_col0, col0 = at.col0;
    const int tile_cols = KSP_RUN << tile_shift;
    const int run = at.run, slot = at.slot, slots = at.slots;
    const int valid = at.valid;  // (0: the lane only helps to stage)

    // Sources s0 .. s0 + n - 1 of the tile into LDS; columns beyond the row are +0 and never
    // read from memory. Consecutive threads take consecutive baselines of one source.
    auto stage = [&](int s0, int n) {
        for (int e = tid; e < n * tile_cols; e += PR_THREADS) {
            const int s = e >> (tile_shift + 4), col = e & (tile_cols - 1);
            const long long c = tile_col0 + col;
            staged[s * (PR_TILE_RUNS * KSP_RUN) + (col & (KSP_RUN - 1)) * PR_TILE_RUNS +
                   (col >> 4)] = c < baselines ? delays[(s0 + s) * delays_stride + c] : 0.0;
        }
    };
    const bool one_block = n_sources <= PR_BLOCK;
    if (one_block) {
        stage(0, n_sources);
        __syncthreads();
    }

    for (long long base = row_begin; base < row_end; base += slots) {
        const long long row = base + slot;
        const bool live = row < row_end && valid > 0;
        double re[KSP_RUN], im[KSP_RUN];
#pragma unroll
        for (int i = 0; i < KSP_RUN; i++) re[i] = im[i] = 0.0;
        const double f = live ? freqs[row] : 0.0;
        for (int s0 = 0; s0 < n_sources; s0 += PR_BLOCK) {
            const int n = min(PR_BLOCK, n_sources - s0);
            if (!one_block) {
                __syncthreads();  // (everyone is done with the block before)
                stage(s0, n);
                __syncthreads();
            }
            if (live) {
                const float *row_flux = flux + row * flux_stride + s0;
                for (int s = 0; s < n; s++) {
                    const double F = (double)row_flux[s];
                    const double *d = staged + s * (PR_TILE_RUNS * KSP_RUN) + run;
#pragma unroll
                    for (int i = 0; i < KSP_RUN; i++) {
                        double co, si;
                        ksp_cos_sin_turns(__dmul_rn(f, d[i * PR_TILE_RUNS]), co, si);
                        re[i] = __dadd_rn(re[i], __dmul_rn(F, co));
                        im[i] = __dsub_rn(im[i], __dmul_rn(F, si));
                    }
                }
            }
        }
        if (!live) continue;

        float2 m[KSP_RUN];
#pragma unroll
        for (int i = 0; i < KSP_RUN; i++) m[i] = make_float2((float)re[i], (float)im[i]);
        if (HAS_M) ksp_run_store(model + row * model_stride + col0, valid, wide, m);
        if (HAS_V) {
            float2 v[KSP_RUN];
            float w[KSP_RUN];
            ksp_run_bytes fl = {0, 0, 0, 0};
            ksp_run_load(vis + row * vis_stride + col0, valid, wide, v, make_float2(0, 0));
            if (HAS_W) ksp_run_load(weights + row * weights_stride + col0, valid, wide, w, 0.0f);
            if (HAS_F) fl = ksp_run_load_bytes(flags + row * flags_stride + col0, valid, wide);
            unsigned bad = 0;
#pragma unroll
            for (int i = 0; i < KSP_RUN; i++) {
                const float mr = m[i].x, mi = m[i].y;
                const float d = ksp_norm2(m[i]);
                const bool ok = d > 0.0f && d < INFINITY;
                // (ksp_cmul_conj(v[i], m[i]) written out: through the helper the compiler allots
                // other registers to three of the variants, 120 to 132 for one)
                const float nr = __fadd_rn(__fmul_rn(v[i].x, mr), __fmul_rn(v[i].y, mi));
                const float ni = __fsub_rn(__fmul_rn(v[i].y, mr), __fmul_rn(v[i].x, mi));
                v[i].x = ok ? __fdiv_rn(nr, d) : v[i].x;
                v[i].y = ok ? __fdiv_rn(ni, d) : v[i].y;
                if (HAS_W) w[i] = ok ? __fmul_rn(w[i], d) : 0.0f;
                bad |= (unsigned)!ok << i;
            }
            ksp_run_store(out_vis + row * out_vis_stride + col0, valid, wide, v);
            if (HAS_W) ksp_run_store(out_weights + row * out_weights_stride + col0, valid, wide, w);
            if (HAS_F) {
                ksp_flag_spread(fl, bad, flag_value);
                ksp_run_store_bytes(out_flags + row * out_flags_stride + col0, valid, wide, fl);
            }
        }
    }
}

extern "C" int ksp_predict(int device, void *stream, const double *freqs, const double *delays,
                           const float *flux, void *model, const void *vis, const float *weights,
                           const uint8_t *flags, void *out_vis, float *out_weights,
                           uint8_t *out_flags, int channels, int baselines, int n_sources,
                           int delays_stride, int flux_stride, int model_stride, int vis_stride,
                           int weights_stride, int flags_stride, int out_vis_stride,
                           int out_weights_stride, int out_flags_stride, int flag_value)
{
    const ksp_plane p_freqs = {"freqs", freqs, 0, 8}, p_delays = {"delays", delays, delays_stride, 8};
    const ksp_plane p_flux = {"flux", flux, flux_stride, 4};
    const ksp_plane p_model = {"model", model, model_stride, 8, true};
    const ksp_plane p_vis = {"vis", vis, vis_stride, 8, true};
    const ksp_plane p_out_vis = {"out_vis", out_vis, out_vis_stride, 8, true};
    const ksp_plane p_weights = {"weights", weights, weights_stride, 4, true};
    const ksp_plane p_out_weights = {"out_weights", out_weights, out_weights_stride, 4, true};
    const ksp_plane p_flags = {"flags", flags, flags_stride, 1, true};
    const ksp_plane p_out_flags = {"out_flags", out_flags, out_flags_stride, 1, true};
    const ksp_planes data = {p_vis, p_out_vis, p_weights, p_out_weights, p_flags, p_out_flags};
    KSP_TRY(ksp_planes_given({p_freqs, p_delays, p_flux}));
    KSP_REQUIRE(model != nullptr || vis != nullptr, "model and vis must not both be NULL");
    KSP_TRY(ksp_pairs_given_together(data));
    KSP_REQUIRE(weights == nullptr || vis != nullptr, "weights needs vis");
    KSP_REQUIRE(flags == nullptr || vis != nullptr, "flags needs vis");
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_sources >= 1 && n_sources <= PR_MAX_SOURCES, "n_sources must be 1..64");
    KSP_REQUIRE(flag_value >= 1 && flag_value <= 255, "flag_value must be 1..255");
    KSP_TRY(ksp_planes_hold({p_delays}, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold({p_flux}, n_sources, "n_sources"));
    KSP_TRY(ksp_planes_hold({p_model}, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold(data, baselines, "baselines"));
    KSP_TRY(ksp_pairs_same_or_apart(data, channels, baselines));
    if (model != nullptr) {
        KSP_REQUIRE(ksp_planes_apart(p_model, channels, baselines, p_freqs, 1, channels),
                    "model overlaps freqs");
        KSP_REQUIRE(ksp_planes_apart(p_model, channels, baselines, p_delays, n_sources, baselines),
                    "model overlaps delays");
        KSP_REQUIRE(ksp_planes_apart(p_model, channels, baselines, p_flux, channels, n_sources),
                    "model overlaps flux");
        for (const ksp_plane &other : data)
            if (other.ptr != nullptr &&
                !ksp_planes_apart(p_model, channels, baselines, other, channels, baselines)) {
                ksp_set_error("invalid argument: model overlaps %s", other.name);
                return (int)hipErrorInvalidValue;
            }
    }
    const ksp_tile_geometry geom =
        ksp_make_tile_geometry(channels, baselines, PR_THREADS, PR_TILE_RUNS, PR_TARGET_GROUPS);
    KSP_REQUIRE(geom.groups <= 0x7fffffffll, "array too large for one launch");
    const bool wide = ksp_planes_aligned({p_model}) && ksp_planes_aligned(data);

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int variant = (model != nullptr ? PR_MODEL : 0) | (vis != nullptr ? PR_DIVIDE : 0) |
                        (weights != nullptr ? PR_WEIGHTS : 0) | (flags != nullptr ? PR_FLAGS : 0);
    ksp_dispatch_exact<1, 2, 3, 6, 7, 10, 11, 14, 15>(variant, [&](auto V) {
        hipLaunchKernelGGL((predict_kernel<V()>), dim3((unsigned)geom.groups), dim3(PR_THREADS), 0,
                           s, freqs, delays, flux, (float2 *)model, (const float2 *)vis, weights,
                           flags, (float2 *)out_vis, out_weights, out_flags, channels, baselines,
                           n_sources, geom.tiles, geom.tile_shift, geom.chunk,
                           (long long)delays_stride, (long long)flux_stride,
                           (long long)model_stride, (long long)vis_stride,
                           (long long)weights_stride, (long long)flags_stride,
                           (long long)out_vis_stride, (long long)out_weights_stride,
                           (long long)out_flags_stride, (unsigned)flag_value, wide);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
