// average_block: a block of 1..8 dumps added to the accumulators of average.hip in one launch.
// The arithmetic is that kernel's, dump after dump: for every sample, and for d = 0 ..
// n_dumps - 1 in that order,
//
//   f = flags[d] | input_flags[d];  we = f ? w[d] * 2^-64 : w[d];
//   acc_vis += we * vis[d] (re and im apart);  acc_weights += we;  acc_flags |= f
//
// each step one float32 operation (-ffp-contract=off, __fmul_rn / __fadd_rn), so the result is
// bit for bit what n_dumps calls of ksp_average_accumulate, or of rfi/host.py AveragerHost.add,
// leave. What the block saves is traffic: the accumulators, 26 of the 39 bytes a sample costs
// per dump, are read once and written once per block, 13 D + 26 bytes instead of 39 D.
//
// Layout: that of average.hip. All arrays are [channels][stride], a lane owns a run of 16
// adjacent baselines of one row, runs are dealt row by row to a one-dimensional grid and the row
// bases are 64-bit. When every pointer of every dump and every row start is 16-byte aligned, a
// run that lies wholly inside its row moves with 16-byte loads and stores; the run at the end
// of a row, and every run of an unaligned call, goes element by element. Either way the lane
// loads its accumulators once and stores them once. Padding is neither read nor written.
//
// The dumps are separate buffers. Their pointers arrive by value in one kernel argument
// (avgb_ptrs) that is indexed with constants only: avgb_pick() compares the dump number, which
// is the same in every lane, with 0 .. 7 in turn, so the pointers of a dump are scalar loads
// from the argument segment and scalar selects, and nothing is copied to scratch memory. One
// row stride per kind serves all dumps: the offset of a run is computed once per kind.
//
// Loads in flight: the walk over the dumps is a rolled loop, and a step issues the 13 (14 with a
// FULL mask) 16-byte loads of its dump together, then adds the dump while they arrive. The
// accumulators and one run are what a lane ever holds, whatever n_dumps is, and three wavefronts
// per SIMD, each at a dump of its own, keep the loads of three dumps in flight there. The
// kernel asks for exactly that occupancy: without the request the scheduler trades the loads in
// flight for registers and waits for every load on its own. (Unrolled over the dumps, by a
// template on their number, the compiler moved the loads of every dump to the top: all 256
// registers from 6 dumps on, and scratch when held to fewer. A second run in the lane, loaded a
// dump ahead, came out with a wait for everything in front of each step's loads. Both are in
// profiles/average_block.md.) No LDS, no workspace, no scratch.
#include "launch.h"

#define AVGB_THREADS 256
#define AVGB_RUN 16
#define AVGB_MAX_DUMPS 8

#define AVGB_FLAGGED_SCALE 0x1p-64f

struct avgb_ptrs {
    const float2 *vis[AVGB_MAX_DUMPS];
    const uint8_t *flags[AVGB_MAX_DUMPS];
    const float *weights[AVGB_MAX_DUMPS];
    const uint8_t *input_flags[AVGB_MAX_DUMPS];
};

// The arrays of one dump.
struct avgb_dump {
    const float2 *vis;
    const uint8_t *flags;
    const float *weights;
    const uint8_t *input_flags;
};

// Dump `d` (wavefront-uniform, 0 .. 7) of `p`.
template <int D = 0>
__device__ __forceinline__ avgb_dump avgb_pick(const avgb_ptrs &p, int d)
{
    if constexpr (D + 1 < AVGB_MAX_DUMPS) {
        if (d != D) return avgb_pick<D + 1>(p, d);
    }
    return {p.vis[D], p.flags[D], p.weights[D], p.input_flags[D]};
}

// Where the lane's run starts in the arrays of each kind, in elements.
struct avgb_offsets {
    long long vis, flags, weights, input_flags, row;
};

// The run of one dump, in registers: v[j] holds samples 2 j and 2 j + 1 as re, im, re, im;
// f has the flag bytes after the masks.
struct avgb_run {
    float4 v[8], w[4];
    uint4 f;
};

// One sample of the accumulation. `f` is the flag byte after the mask, anywhere in the word.
template <bool HAS_W>
__device__ __forceinline__ void avgb_add(float vre, float vim, float w, unsigned f, float &are,
                                         float &aim, float &aw)
{
    const float w1 = HAS_W ? w : 1.0f;
    const float we = f != 0 ? __fmul_rn(w1, AVGB_FLAGGED_SCALE) : w1;
    are = __fadd_rn(are, __fmul_rn(we, vre));
    aim = __fadd_rn(aim, __fmul_rn(we, vim));
    aw = __fadd_rn(aw, we);
}

// MODE: 0 no input flags, 1 one byte per row, 2 one byte per sample.
template <bool HAS_W, int MODE>
__device__ __forceinline__ void avgb_load(const avgb_dump &dump, const avgb_offsets &o,
                                          avgb_run &x)
{
    const float4 *v = reinterpret_cast<const float4 *>(dump.vis + o.vis);
#pragma unroll
    for (int j = 0; j < 8; j++) x.v[j] = v[j];
    if (HAS_W) {
        const float4 *w = reinterpret_cast<const float4 *>(dump.weights + o.weights);
#pragma unroll
        for (int j = 0; j < 4; j++) x.w[j] = w[j];
    }
    uint4 f = *reinterpret_cast<const uint4 *>(dump.flags + o.flags);
    if (MODE == 2) {
        const uint4 m = *reinterpret_cast<const uint4 *>(dump.input_flags + o.input_flags);
        f = make_uint4(f.x | m.x, f.y | m.y, f.z | m.z, f.w | m.w);
    }
    if (MODE == 1) {
        // the row's mask byte in every byte of a word
        const unsigned m = dump.input_flags[o.row] * 0x01010101u;
        f = make_uint4(f.x | m, f.y | m, f.z | m, f.w | m);
    }
    x.f = f;
}

// The run `x` of one dump onto the accumulators.
template <bool HAS_W>
__device__ __forceinline__ void avgb_add_run(const avgb_run &x, float4 (&av)[8], float4 (&aw)[4],
                                             uint4 &af)
{
    const unsigned fw[4] = {x.f.x, x.f.y, x.f.z, x.f.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 w = HAS_W ? x.w[q] : make_float4(1, 1, 1, 1);
        avgb_add<HAS_W>(x.v[2 * q].x, x.v[2 * q].y, w.x, fw[q] & 0xffu, av[2 * q].x, av[2 * q].y,
                        aw[q].x);
        avgb_add<HAS_W>(x.v[2 * q].z, x.v[2 * q].w, w.y, fw[q] & 0xff00u, av[2 * q].z,
                        av[2 * q].w, aw[q].y);
        avgb_add<HAS_W>(x.v[2 * q + 1].x, x.v[2 * q + 1].y, w.z, fw[q] & 0xff0000u,
                        av[2 * q + 1].x, av[2 * q + 1].y, aw[q].z);
        avgb_add<HAS_W>(x.v[2 * q + 1].z, x.v[2 * q + 1].w, w.w, fw[q] & 0xff000000u,
                        av[2 * q + 1].z, av[2 * q + 1].w, aw[q].w);
    }
    af = make_uint4(af.x | x.f.x, af.y | x.f.y, af.z | x.f.z, af.w | x.f.w);
}

// (three wavefronts per SIMD, no more and no fewer: "Loads in flight" above)
template <bool HAS_W, int MODE>
__global__ __launch_bounds__(AVGB_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3)))
void average_accumulate_block_kernel(
    const avgb_ptrs p, int n_dumps, float2 *__restrict__ acc_vis, float *__restrict__ acc_weights,
    uint8_t *__restrict__ acc_flags, long long runs, int runs_per_row, int baselines,
    int vis_stride, int flags_stride, int weights_stride, int input_flags_stride,
    int acc_vis_stride, int acc_weights_stride, int acc_flags_stride, int aligned)
{
    const long long run = (long long)blockIdx.x * AVGB_THREADS + threadIdx.x;
    if (run >= runs) return;
    const long long row = run / runs_per_row;
    const int col0 = (int)(run - row * runs_per_row) * AVGB_RUN;
    const int valid = min(AVGB_RUN, baselines - col0);  // >= 1

    avgb_offsets o;
    o.vis = row * vis_stride + col0;
    o.flags = row * flags_stride + col0;
    o.weights = row * weights_stride + col0;
    o.input_flags = row * input_flags_stride + col0;
    o.row = row;
    float2 *av = acc_vis + row * acc_vis_stride + col0;
    float *aw = acc_weights + row * acc_weights_stride + col0;
    uint8_t *af = acc_flags + row * acc_flags_stride + col0;

    if (aligned && valid == AVGB_RUN) {
        float4 sv[8], sw[4];
#pragma unroll
        for (int j = 0; j < 8; j++) sv[j] = reinterpret_cast<const float4 *>(av)[j];
#pragma unroll
        for (int j = 0; j < 4; j++) sw[j] = reinterpret_cast<const float4 *>(aw)[j];
        uint4 sf = *reinterpret_cast<const uint4 *>(af);
#pragma unroll 1
        for (int d = 0; d < n_dumps; d++) {
            avgb_run x;
            avgb_load<HAS_W, MODE>(avgb_pick(p, d), o, x);
            avgb_add_run<HAS_W>(x, sv, sw, sf);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) reinterpret_cast<float4 *>(av)[j] = sv[j];
#pragma unroll
        for (int j = 0; j < 4; j++) reinterpret_cast<float4 *>(aw)[j] = sw[j];
        *reinterpret_cast<uint4 *>(af) = sf;
    } else {
        for (int i = 0; i < valid; i++) {
            float2 a = av[i];
            float sw = aw[i];
            unsigned sf = af[i];
#pragma unroll 1
            for (int d = 0; d < n_dumps; d++) {
                const avgb_dump dump = avgb_pick(p, d);
                unsigned f = dump.flags[o.flags + i];
                if (MODE == 1) f |= dump.input_flags[o.row];
                if (MODE == 2) f |= dump.input_flags[o.input_flags + i];
                const float2 z = dump.vis[o.vis + i];
                avgb_add<HAS_W>(z.x, z.y, HAS_W ? dump.weights[o.weights + i] : 1.0f, f, a.x, a.y,
                                sw);
                sf |= f;
            }
            av[i] = a;
            aw[i] = sw;
            af[i] = (uint8_t)sf;
        }
    }
}

extern "C" int ksp_average_accumulate_block(
    int device, void *stream, int n_dumps, const void *const *vis, const uint8_t *const *flags,
    const float *const *weights, const uint8_t *const *input_flags, int input_flags_mode,
    void *acc_vis, float *acc_weights, uint8_t *acc_flags, int channels, int baselines,
    int vis_stride, int flags_stride, int weights_stride, int input_flags_stride,
    int acc_vis_stride, int acc_weights_stride, int acc_flags_stride)
{
    KSP_REQUIRE(n_dumps >= 1 && n_dumps <= AVGB_MAX_DUMPS, "n_dumps must be 1..8");
    KSP_REQUIRE(vis != nullptr, "vis is NULL");
    KSP_REQUIRE(flags != nullptr, "flags is NULL");
    const ksp_planes acc = {{"acc_vis", acc_vis, acc_vis_stride, 8},
                            {"acc_weights", acc_weights, acc_weights_stride, 4},
                            {"acc_flags", acc_flags, acc_flags_stride, 1}};
    KSP_TRY(ksp_planes_given(acc));
    KSP_REQUIRE(input_flags_mode >= 0 && input_flags_mode <= 2,
                "input_flags_mode must be 0 (none), 1 (per channel) or 2 (per sample)");
    KSP_REQUIRE(input_flags_mode == 0 || input_flags != nullptr,
                "input_flags is NULL but input_flags_mode is not 0");
    KSP_REQUIRE(input_flags_mode != 0 || input_flags == nullptr,
                "input_flags given but input_flags_mode is 0");
    for (int d = 0; d < n_dumps; d++) {
        KSP_REQUIRE(vis[d] != nullptr, "an entry of vis is NULL");
        KSP_REQUIRE(flags[d] != nullptr, "an entry of flags is NULL");
        KSP_REQUIRE(weights == nullptr || weights[d] != nullptr, "an entry of weights is NULL");
        KSP_REQUIRE(input_flags == nullptr || input_flags[d] != nullptr,
                    "an entry of input_flags is NULL");
    }
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    // one misaligned pointer of one dump sends the whole call down the element path
    avgb_ptrs p = {};
    int aligned = 1;
    for (int d = 0; d < n_dumps; d++) {
        p.vis[d] = (const float2 *)vis[d];
        p.flags[d] = flags[d];
        p.weights[d] = weights != nullptr ? weights[d] : nullptr;
        p.input_flags[d] = input_flags != nullptr ? input_flags[d] : nullptr;
        // (input_flags has a row stride only as one byte per sample)
        const ksp_planes dump = {
            {"vis", p.vis[d], vis_stride, 8},
            {"flags", p.flags[d], flags_stride, 1},
            {"weights", p.weights[d], weights_stride, 4, true},
            {"input_flags", input_flags_mode == 2 ? p.input_flags[d] : nullptr,
             input_flags_stride, 1, true}};
        KSP_TRY(ksp_planes_hold(dump, baselines, "baselines"));
        aligned = aligned && ksp_planes_aligned(dump);
    }
    KSP_TRY(ksp_planes_hold(acc, baselines, "baselines"));
    aligned = aligned && ksp_planes_aligned(acc);
    ksp_run_grid g;
    KSP_TRY(ksp_make_run_grid(channels, baselines, AVGB_RUN, AVGB_THREADS, g));

    KSP_CHECK(hipSetDevice(device));
    ksp_dispatch_bool(weights != nullptr, [&](auto HAS_W) {
        // (input_flags_mode is 0 .. 2 here)
        ksp_dispatch_exact<0, 1, 2>(input_flags_mode, [&](auto MODE) {
            hipLaunchKernelGGL(
                (average_accumulate_block_kernel<decltype(HAS_W)::value, MODE()>),
                dim3((unsigned)g.groups), dim3(AVGB_THREADS), 0, (hipStream_t)stream, p, n_dumps,
                (float2 *)acc_vis, acc_weights, acc_flags, g.runs, g.runs_per_row, baselines,
                vis_stride, flags_stride, weights_stride, input_flags_stride, acc_vis_stride,
                acc_weights_stride, acc_flags_stride, aligned);
        });
    });
    KSP_LAUNCH_CHECK();
    return 0;
}

