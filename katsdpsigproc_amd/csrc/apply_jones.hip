// apply_jones: per-antenna 2x2 Jones corrections applied to visibilities, weights and flags,
// C_a V_ab C_b^H on the four products of an antenna pair, in one launch (no reference
// counterpart). rfi/host.py ApplyJonesHost is the definition and states every step; the kernel
// reproduces it bit for bit, so every float step below is one float32 operation (the
// translation unit is built with -ffp-contract=off and correctly rounded division, and the
// steps are written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, which are never
// contracted; the complex products are those of cal_math.h).
//
//   per channel c and quad q, with (a, b) = quad_antennas[q], (t00, t01, t10, t11) = quads[q]:
//     an entry t is present when t != 0 and |t| <= baselines: baseline |t| - 1, conjugated on
//     load and on store when t < 0; with a == b an absent (1,0) beside a present (0,1) reads
//     as its conjugate, and the other way round
//     complete = 0 <= a, b < n_inputs / 2 and all four sources are there
//     ok = complete and none of the 16 floats of rows 2a, 2a+1, 2b, 2b+1 of jones[c] is NaN
//     T[i][n] = C_a[i][0] S[0][n] + C_a[i][1] S[1][n]
//     O[i][k] = T[i][0] conj(C_b[k][0]) + T[i][1] conj(C_b[k][1])
//     u[i][n] = |C_a[i][0]|^2 (1 / w[0][n]) + |C_a[i][1]|^2 (1 / w[1][n])
//     var[i][k] = u[i][0] |C_b[k][0]|^2 + u[i][1] |C_b[k][1]|^2
//     for the present entries: out_vis = ok ? O[i][k] : vis;
//     out_weights = ok and every w > 0 and var > 0 ? 1 / var : 0;
//     out_flags = OR of the present flags | (ok ? 0 : flag_value)
//
// Layout. The six sample arrays are [channels][stride] with baselines contiguous. A lane owns a
// quad: it keeps the quad's six table integers in registers for as long as it lives (as
// apply_gains keeps its indices), and per row it loads the up to four samples of every array,
// works out the four products and stores them. Consecutive lanes take consecutive quads, so
// with the baselines in polarisation blocks each of the four 8-byte loads and stores is
// contiguous across the wavefront, and with the four products of a pair adjacent a lane moves
// 32 adjacent bytes. The rows of jones (16 bytes per input) are gathered through LDS as
// apply_gains gathers its gains: a workgroup copies whole rows of `jones` into AJ_LDS_ROWS =
// 2048 slots of 16 bytes (32 KiB), as many rows of the array as fit (aj_stage_rows, which
// depends on n_inputs alone), and every lane then picks its four rows with 16-byte LDS reads:
// 16 bytes of LDS reads per sample, as there. The copy itself is made in complex64 elements,
// which is all the alignment `jones` promises.
//
// Geometry (its own: tile_grid.h counts in runs of 16 baselines, this one in quads). A
// workgroup of 256 threads owns a tile of `tile_quads` quads (a power of two, 1 .. 256: the
// narrowest that holds the table) and a chunk of `chunk` rows, about AJ_TARGET_GROUPS
// workgroups to a launch: thread t owns quad t % tile_quads of the tile and, of each stage, the
// rows t / tile_quads, t / tile_quads + 256 / tile_quads, ... A workgroup walks its chunk in
// stages of at most aj_stage_rows rows, two barriers per stage. Row bases are 64-bit.
//
// In place. A lane loads every source of every array of a row before it stores any of them,
// and a baseline belongs to one entry of one quad (the caller's promise), so an output may be
// its input (same pointer, same stride). The sample pointers are therefore not __restrict__.
//
// Traffic per sample: 8 + 4 + 1 bytes read and as many written, 26 in all (24, 18 and 16
// without flags, weights or both); per lane 24 bytes of table; per workgroup and stage the rows
// of jones it stages, which come from L2 for all but the first workgroup to ask.
#include "cal_math.h"
#include "launch.h"

#define AJ_THREADS 256
#define AJ_LDS_ROWS 2048        // rows of jones a stage holds (16 bytes each)
#define AJ_MAX_INPUTS 2048      // so one row of the array always fits
#define AJ_STAGE_ROWS_MAX 256   // no stage is taller (one row per thread)
#ifndef AJ_TARGET_GROUPS  // (an experiment's -D, KSP_EXTRA_HIPCC_FLAGS)
#define AJ_TARGET_GROUPS 1024
#endif

// Rows of the array per stage (tests/test_gpu_apply_jones.py has the same formula)
static int aj_stage_rows(int n_inputs)
{
    const int fit = AJ_LDS_ROWS / n_inputs;
    return fit < AJ_STAGE_ROWS_MAX ? fit : AJ_STAGE_ROWS_MAX;
}

// The grid: what the launcher works out (tests/test_gpu_apply_jones.py has the same formulas)
struct aj_geometry {
    int tile_shift;  // log2(tile_quads)
    int tiles;       // tiles to the table
    int chunk;       // rows per workgroup
    long long groups;
};

// (groups stays below 3 * AJ_TARGET_GROUPS + tiles, and tiles is at most 2^31 / 256)
static aj_geometry aj_make_geometry(int channels, int n_quads)
{
    aj_geometry g;
    g.tile_shift = 0;
    while ((1 << g.tile_shift) < AJ_THREADS && (1 << g.tile_shift) < n_quads) g.tile_shift++;
    const int tile_quads = 1 << g.tile_shift;
    g.tiles = (int)(((long long)n_quads + tile_quads - 1) / tile_quads);
    const int slots = AJ_THREADS / tile_quads;  // rows a workgroup works on at once
    long long chunk = (long long)channels * g.tiles / AJ_TARGET_GROUPS / slots * slots;
    if (chunk > channels) chunk = channels;  // (long tables: the tiles alone are groups enough)
    if (chunk < slots) chunk = slots;
    g.chunk = (int)chunk;
    g.groups = (channels + chunk - 1) / chunk * g.tiles;
    return g;
}

// The sign of x flipped where `flip` (exactly: twice gives x's bits back, a NaN's included)
__device__ __forceinline__ float aj_flip(float x, bool flip)
{
    return __uint_as_float(__float_as_uint(x) ^ (flip ? 0x80000000u : 0u));
}

template <bool HAS_W, bool HAS_F>
__global__ __launch_bounds__(AJ_THREADS) void apply_jones_kernel(
    const float2 *vis, const float *weights, const uint8_t *flags,
    const float2 *__restrict__ jones, const int *__restrict__ quad_antennas,
    const int *__restrict__ quads, float2 *out_vis, float *out_weights, uint8_t *out_flags,
    int channels, int baselines, int n_inputs, int n_quads, int tiles, int tile_shift, int chunk,
    int stage_rows, long long vis_stride, long long weights_stride, long long flags_stride,
    long long jones_stride, long long out_vis_stride, long long out_weights_stride,
    long long out_flags_stride, unsigned flag_value)
{
    __shared__ float4 staged[AJ_LDS_ROWS];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles;
    const long long row_begin = (long long)(blockIdx.x / tiles) * chunk;
    const long long row_end = min((long long)channels, row_begin + chunk);
    const int slot = tid >> tile_shift, slots = AJ_THREADS >> tile_shift;
    const long long quad = ((long long)tile << tile_shift) + (tid & ((1 << tile_shift) - 1));
    const bool valid = quad < n_quads;  // (false: the lane only helps to stage)

    // The lane's quad, once: where its four sources are (`have`), which of them are entries of
    // its own (`present`: loaded and stored), which are conjugated (`neg`), and its two
    // antennas, replaced by 0 and remembered when one is outside 0 .. n_inputs / 2 - 1.
    int j[4] = {0, 0, 0, 0};
    unsigned present = 0, neg = 0;
    int ant_a = 0, ant_b = 0;
    bool complete = false, stand1 = false, stand2 = false;
    if (valid) {
        const int a = quad_antennas[2 * quad], b = quad_antennas[2 * quad + 1];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int t = quads[4 * quad + e];
            // (|t| as unsigned: INT32_MIN has none as an int)
            const unsigned mag = t < 0 ? 0u - (unsigned)t : (unsigned)t;
            const bool in = mag - 1u < (unsigned)baselines;  // (t == 0 wraps to 2^32 - 1)
            present |= (unsigned)in << e;
            neg |= (unsigned)(in && t < 0) << e;
            j[e] = in ? (int)(mag - 1u) : 0;
        }
        stand1 = a == b && (present & 6u) == 4u;  // (1,0) stands in for (0,1)
        stand2 = a == b && (present & 6u) == 2u;  // (0,1) stands in for (1,0)
        const unsigned have = present | (stand1 ? 2u : 0u) | (stand2 ? 4u : 0u);
        const unsigned n_ant = (unsigned)n_inputs >> 1;
        const bool inr = (unsigned)a < n_ant && (unsigned)b < n_ant;
        complete = inr && have == 15u;
        ant_a = inr ? a : 0;
        ant_b = inr ? b : 0;
    }

    // Staging walks the flat index of (row of the stage, complex64 of the row) in steps of the
    // workgroup: a row of the array is 2 * n_inputs complex64
    const float2 *jones2 = jones;
    float2 *staged2 = reinterpret_cast<float2 *>(staged);
    const int row_len = 2 * n_inputs;
    const int stage_r0 = tid / row_len, stage_c0 = tid - stage_r0 * row_len;
    const int stage_dr = AJ_THREADS / row_len, stage_dc = AJ_THREADS - stage_dr * row_len;

    for (long long s = row_begin; s < row_end; s += stage_rows) {
        const int n = (int)min((long long)stage_rows, row_end - s);  // n * n_inputs <= AJ_LDS_ROWS
        for (int r = stage_r0, c = stage_c0, e = tid; r < n; e += AJ_THREADS) {
            staged2[e] = jones2[(s + r) * (2 * jones_stride) + c];
            r += stage_dr;
            c += stage_dc;
            if (c >= row_len) {
                c -= row_len;
                r++;
            }
        }
        __syncthreads();
        if (valid) {
            for (int r = slot; r < n; r += slots) {
                const long long row = s + r;
                const float4 *g = staged + r * n_inputs;
                // every source of every array, before any store
                float2 raw[4];
                float w[4];
                unsigned any_f = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    raw[e] = make_float2(0.0f, 0.0f);
                    w[e] = 1.0f;
                    if ((present >> e) & 1u) {
                        raw[e] = vis[row * vis_stride + j[e]];
                        if (HAS_W) w[e] = weights[row * weights_stride + j[e]];
                        if (HAS_F) any_f |= flags[row * flags_stride + j[e]];
                    }
                }
                float2 src[4];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    src[e] = make_float2(raw[e].x, aj_flip(raw[e].y, (neg >> e) & 1u));
                if (stand1) {
                    src[1] = make_float2(src[2].x, aj_flip(src[2].y, true));
                    w[1] = w[2];
                }
                if (stand2) {
                    src[2] = make_float2(src[1].x, aj_flip(src[1].y, true));
                    w[2] = w[1];
                }
                const float4 a0 = g[2 * ant_a], a1 = g[2 * ant_a + 1];
                const float4 b0 = g[2 * ant_b], b1 = g[2 * ant_b + 1];
                // C_a[i][m] and C_b[k][n]
                const float2 ca[2][2] = {{make_float2(a0.x, a0.y), make_float2(a0.z, a0.w)},
                                         {make_float2(a1.x, a1.y), make_float2(a1.z, a1.w)}};
                const float2 cb[2][2] = {{make_float2(b0.x, b0.y), make_float2(b0.z, b0.w)},
                                         {make_float2(b1.x, b1.y), make_float2(b1.z, b1.w)}};
                bool nan = false;
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int m = 0; m < 2; m++)
                        nan = nan || __builtin_isnan(ca[i][m].x) || __builtin_isnan(ca[i][m].y) ||
                              __builtin_isnan(cb[i][m].x) || __builtin_isnan(cb[i][m].y);
                const bool ok = complete && !nan;
                float2 out[4];
                float var[4];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const float2 t0 = ksp_cadd(ksp_cmul(ca[i][0], src[0]), ksp_cmul(ca[i][1], src[2]));
                    const float2 t1 = ksp_cadd(ksp_cmul(ca[i][0], src[1]), ksp_cmul(ca[i][1], src[3]));
#pragma unroll
                    for (int k = 0; k < 2; k++)
                        out[2 * i + k] = ksp_row_dot_conj(t0, t1, cb[k][0], cb[k][1]);
                }
                bool all_w = true;
                if (HAS_W) {
                    float rw[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        all_w = all_w && w[e] > 0.0f;
                        rw[e] = __fdiv_rn(1.0f, w[e]);
                    }
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const float al0 = ksp_norm2(ca[i][0]), al1 = ksp_norm2(ca[i][1]);
                        const float u0 = __fadd_rn(__fmul_rn(al0, rw[0]), __fmul_rn(al1, rw[2]));
                        const float u1 = __fadd_rn(__fmul_rn(al0, rw[1]), __fmul_rn(al1, rw[3]));
#pragma unroll
                        for (int k = 0; k < 2; k++)
                            var[2 * i + k] = __fadd_rn(__fmul_rn(u0, ksp_norm2(cb[k][0])),
                                                       __fmul_rn(u1, ksp_norm2(cb[k][1])));
                    }
                }
                const unsigned f_out = any_f | (ok ? 0u : flag_value);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if ((present >> e) & 1u) {
                        const float2 o = make_float2(out[e].x, aj_flip(out[e].y, (neg >> e) & 1u));
                        out_vis[row * out_vis_stride + j[e]] = ok ? o : raw[e];
                        if (HAS_W)
                            out_weights[row * out_weights_stride + j[e]] =
                                ok && all_w && var[e] > 0.0f ? __fdiv_rn(1.0f, var[e]) : 0.0f;
                        if (HAS_F) out_flags[row * out_flags_stride + j[e]] = (uint8_t)f_out;
                    }
                }
            }
        }
        __syncthreads();
    }
}

extern "C" int ksp_apply_jones(int device, void *stream, const void *vis, const float *weights,
                               const uint8_t *flags, const void *jones,
                               const int32_t *quad_antennas, const int32_t *quads, void *out_vis,
                               float *out_weights, uint8_t *out_flags, int channels, int baselines,
                               int n_inputs, int n_quads, int vis_stride, int weights_stride,
                               int flags_stride, int jones_stride, int out_vis_stride,
                               int out_weights_stride, int out_flags_stride, int flag_value)
{
    const ksp_plane in = {"vis", vis, vis_stride, 8}, out = {"out_vis", out_vis, out_vis_stride, 8};
    // (an element of jones is a row of two complex64)
    const ksp_plane table = {"jones", jones, jones_stride, 16};
    const ksp_planes pairs = {{"weights", weights, weights_stride, 4, true},
                              {"out_weights", out_weights, out_weights_stride, 4, true},
                              {"flags", flags, flags_stride, 1, true},
                              {"out_flags", out_flags, out_flags_stride, 1, true}};
    KSP_TRY(ksp_planes_given(
        {in, table, {"quad_antennas", quad_antennas, 0, 4}, {"quads", quads, 0, 4}, out}));
    KSP_TRY(ksp_pairs_given_together(pairs));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_inputs >= 2 && n_inputs <= AJ_MAX_INPUTS && n_inputs % 2 == 0,
                "n_inputs must be even and 2..2048");
    KSP_REQUIRE(n_quads >= 1, "n_quads must be at least 1");
    KSP_REQUIRE(flag_value >= 1 && flag_value <= 255, "flag_value must be 1..255");
    KSP_TRY(ksp_planes_hold({in, out}, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold({table}, n_inputs, "n_inputs"));
    KSP_TRY(ksp_planes_hold(pairs, baselines, "baselines"));
    KSP_TRY(ksp_pairs_same_or_apart({in, out}, channels, baselines));
    KSP_TRY(ksp_pairs_same_or_apart(pairs, channels, baselines));
    const aj_geometry geom = aj_make_geometry(channels, n_quads);
    KSP_REQUIRE(geom.groups <= 0x7fffffffll, "array too large for one launch");

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int variant = (weights != nullptr ? 1 : 0) | (flags != nullptr ? 2 : 0);
    ksp_dispatch_exact<0, 1, 2, 3>(variant, [&](auto V) {
        hipLaunchKernelGGL((apply_jones_kernel<(V() & 1) != 0, (V() & 2) != 0>),
                           dim3((unsigned)geom.groups), dim3(AJ_THREADS), 0, s, (const float2 *)vis,
                           weights, flags, (const float2 *)jones, (const int *)quad_antennas,
                           (const int *)quads, (float2 *)out_vis, out_weights, out_flags, channels,
                           baselines, n_inputs, n_quads, geom.tiles, geom.tile_shift, geom.chunk,
                           aj_stage_rows(n_inputs), (long long)vis_stride,
                           (long long)weights_stride, (long long)flags_stride,
                           (long long)jones_stride, (long long)out_vis_stride,
                           (long long)out_weights_stride, (long long)out_flags_stride,
                           (unsigned)flag_value);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
