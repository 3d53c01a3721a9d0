// solve_gains: per-input complex gains solved from averaged visibilities, channel by channel,
// with StEFCal, in one launch (no reference counterpart). rfi/host.py SolveGainsHost is the
// definition; the kernel reproduces it bit for bit, so every float step below is one float32
// operation (the translation unit is built with -ffp-contract=off and correctly rounded
// division and square root, and the steps are written with __fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn, which are never contracted; the one square root is __builtin_sqrtf, which that
// build flag expands to the correctly rounded sequence, where __fsqrt_rn is the bare
// instruction, good to 1 ulp), and every sum runs in the host's order:
// blocks of SG_BLOCK = 32 indices, sequential and ascending from +0 inside a block, the block
// sums added in ascending order.
//
//   per channel, with A and W as below, g = initial or 1, for k = 1 .. max_iterations:
//     s[q]   = g[q].re g[q].re + g[q].im g[q].im
//     num[p] = sum_q (A.re g.re - A.im g.im, A.re g.im + A.im g.re)      (A = A[p][q], g = g[q])
//     den[p] = sum_q W[p][q] s[q]
//     new[p] = den[p] > 0 ? num[p] / den[p] : g[p]
//     k odd:  g = new;    k even: g = (new + g) * 0.5, and stop when
//     sum_p |g[p] - old[p]|^2 <= tol2 * sum_p |g[p]|^2          (p over the inputs with data)
//   then referencing, corrections and NaN for the inputs without data.
//
// One workgroup per channel. Load phase: the threads walk the upper triangle of `pairs` (the
// same table for every channel: from L2 after the first), gather the samples the entries name
// and fill LDS with the upper triangle of A and W, 12 bytes per pair (three float arrays of
// n (n - 1) / 2 elements: 97536 bytes at 128 inputs). An entry is validated before anything is
// derived from it: 0, or one whose magnitude exceeds `baselines` (INT32_MIN included, compared
// without negating it), forms no address: its thread reads baseline 0 instead, which always
// exists, and drops it, so that a thread's loads need no branch and SG_UNROLL = 8 elements are
// in flight at once (first their entries, then their samples).
// Iteration phase: thread (p, b) sums block b of row p,
// reading element (p, q) from the triangle, conjugated below the diagonal and +0 on it; thread p
// then adds the block sums and updates g[p] (phase 1 has finished: nobody reads the old g any
// more); on even k thread b sums block b of the two p-sums and every thread adds the block sums
// and takes the same decision. Two barriers per odd iteration, three per even one. The loop
// count depends on the channel's data and is uniform over the workgroup.
//
// The workgroup has n * ceil(n / 32) threads rounded up to whole wavefronts: 64 for up to 32
// inputs, 128 for 64, 512 for 128. No atomics, no workspace, no dependence on the order of
// workgroups. The sample arrays have any row stride; padding is neither read nor written.
#include "cal_math.h"
#include "launch.h"

#define SG_MAX_INPUTS 128
#define SG_MAX_ITERATIONS 1000
#define SG_BLOCK 32
#define SG_UNROLL 8  // elements of the triangle a thread loads at once
#define SG_MAX_BLOCKS (SG_MAX_INPUTS / SG_BLOCK)
#define SG_NOT_CONVERGED 1
#define SG_NO_DATA 2
#define SG_NOT_REFERENCED 4

static int sg_blocks(int n_inputs) { return (n_inputs + SG_BLOCK - 1) / SG_BLOCK; }
static int sg_threads(int n_inputs) { return (n_inputs * sg_blocks(n_inputs) + 63) / 64 * 64; }
// Elements of a triangle array (one even for a single input, whose diagonal read is discarded)
static int sg_pairs(int n_inputs)
{
    const int pairs = n_inputs * (n_inputs - 1) / 2;
    return pairs > 0 ? pairs : 1;
}
// Dynamic LDS in 4-byte words: three triangles; g.re, g.im and s per input; three block sums
// per (block, input); the two p-terms and the data mark per input; the block sums of the p-sums
static size_t sg_lds_words(int n_inputs)
{
    return 3 * (size_t)sg_pairs(n_inputs) + 3 * (size_t)n_inputs +
           3 * (size_t)sg_blocks(n_inputs) * n_inputs + 3 * (size_t)n_inputs + 2 * SG_MAX_BLOCKS;
}

struct sg_strides {
    long long vis, weights, flags, pairs, initial, gains;
};

template <bool HAS_W, bool HAS_F, bool HAS_I>
__global__ __launch_bounds__(512) void solve_gains_kernel(
    const float2 *__restrict__ vis, const float *__restrict__ weights,
    const uint8_t *__restrict__ flags, const int *__restrict__ pairs, const float2 *initial,
    float2 *gains, int *__restrict__ iterations, uint8_t *__restrict__ status, int baselines, int n,
    sg_strides stride, int max_iterations, float tol2, int reference, unsigned mask,
    int corrections)
{
    extern __shared__ float sg_lds[];
    const int tid = threadIdx.x, threads = blockDim.x;
    const long long c = blockIdx.x;
    const int n_pairs = n * (n - 1) / 2, n_alloc = n_pairs > 0 ? n_pairs : 1;
    const int blocks = (n + SG_BLOCK - 1) / SG_BLOCK;
    float *a_re = sg_lds, *a_im = a_re + n_alloc, *a_w = a_im + n_alloc;
    float *g_re = a_w + n_alloc, *g_im = g_re + n, *g_s = g_im + n;
    float *part_re = g_s + n, *part_im = part_re + blocks * n, *part_den = part_im + blocks * n;
    float *d_term = part_den + blocks * n, *n_term = d_term + n;
    int *has = reinterpret_cast<int *>(n_term + n);
    float *d_part = reinterpret_cast<float *>(has + n), *n_part = d_part + SG_MAX_BLOCKS;

    // ---- load: g, the data marks, then the triangle
    if (tid < n) {
        float2 g0 = make_float2(1.0f, 0.0f);
        if (HAS_I) g0 = initial[c * stride.initial + tid];
        g_re[tid] = g0.x;
        g_im[tid] = g0.y;
        g_s[tid] = ksp_norm2(g0);
        has[tid] = 0;
    }
    __syncthreads();
    {
        // SG_UNROLL elements per trip, all their loads in flight together: first the entries of
        // `pairs`, then the samples they name. An entry that is no baseline reads baseline 0
        // instead (which exists) and its sample is dropped.
        int p = 0, row = 0;  // row: the flat index of (p, p + 1)
        for (int e0 = tid; e0 < n_pairs; e0 += SG_UNROLL * threads) {
            int pp[SG_UNROLL], qq[SG_UNROLL], t[SG_UNROLL];
#pragma unroll
            for (int u = 0; u < SG_UNROLL; u++) {
                const int e = e0 + u * threads;
                pp[u] = -1;
                if (e < n_pairs) {
                    while (e >= row + (n - 1 - p)) {
                        row += n - 1 - p;
                        p++;
                    }
                    pp[u] = p;
                    qq[u] = p + 1 + (e - row);
                }
            }
#pragma unroll
            for (int u = 0; u < SG_UNROLL; u++)
                t[u] = pp[u] >= 0 ? pairs[pp[u] * stride.pairs + qq[u]] : 0;
            float2 v[SG_UNROLL];
            float ws[SG_UNROLL];
            unsigned f[SG_UNROLL];
            bool valid[SG_UNROLL];
#pragma unroll
            for (int u = 0; u < SG_UNROLL; u++) {
                valid[u] = t[u] > 0 ? t[u] <= baselines : (t[u] < 0 && t[u] >= -baselines);
                const long long at = valid[u] ? (t[u] > 0 ? t[u] : -t[u]) - 1 : 0;
                v[u] = vis[c * stride.vis + at];
                ws[u] = HAS_W ? weights[c * stride.weights + at] : 1.0f;
                f[u] = HAS_F ? flags[c * stride.flags + at] : 0u;
            }
#pragma unroll
            for (int u = 0; u < SG_UNROLL; u++) {
                if (pp[u] < 0) continue;
                const bool kept = valid[u] && !__builtin_isnan(v[u].x) &&
                                  !__builtin_isnan(v[u].y) && ws[u] > 0.0f && (f[u] & mask) == 0;
                float re = 0.0f, im = 0.0f, w = 0.0f;
                if (kept) {
                    re = __fmul_rn(ws[u], v[u].x);
                    im = __fmul_rn(ws[u], v[u].y);
                    if (t[u] < 0) im = -im;
                    w = ws[u];
                    has[pp[u]] = 1;  // (every writer stores the same value)
                    has[qq[u]] = 1;
                }
                const int e = e0 + u * threads;
                a_re[e] = re;
                a_im[e] = im;
                a_w[e] = w;
            }
        }
    }
    __syncthreads();

    // ---- iterate
    const int b = tid / n, p = tid - b * n;  // thread (p, b); b >= blocks: only barriers
    const int q_begin = b * SG_BLOCK, q_end = min(n, q_begin + SG_BLOCK);
    const bool has_p = tid < n && has[tid] != 0;
    int k = 0;
    bool converged = false;
    while (k < max_iterations && !converged) {
        k++;
        if (b < blocks) {
            float nr = 0.0f, ni = 0.0f, dn = 0.0f;
#pragma unroll 4
            for (int q = q_begin; q < q_end; q++) {
                const int lo = min(p, q), hi = max(p, q);
                const bool off = p != q;
                const int e = off ? lo * (2 * n - lo - 1) / 2 + (hi - lo - 1) : 0;
                const float ar = off ? a_re[e] : 0.0f;
                float ai = off ? a_im[e] : 0.0f;
                const float w = off ? a_w[e] : 0.0f;
                if (p > q) ai = -ai;
                const float2 ag = ksp_cmul(make_float2(ar, ai), make_float2(g_re[q], g_im[q]));
                nr = __fadd_rn(nr, ag.x);
                ni = __fadd_rn(ni, ag.y);
                dn = __fadd_rn(dn, __fmul_rn(w, g_s[q]));
            }
            part_re[b * n + p] = nr;
            part_im[b * n + p] = ni;
            part_den[b * n + p] = dn;
        }
        __syncthreads();
        if (tid < n) {
            float nr = part_re[tid], ni = part_im[tid], dn = part_den[tid];
            for (int i = 1; i < blocks; i++) {
                nr = __fadd_rn(nr, part_re[i * n + tid]);
                ni = __fadd_rn(ni, part_im[i * n + tid]);
                dn = __fadd_rn(dn, part_den[i * n + tid]);
            }
            const float old_re = g_re[tid], old_im = g_im[tid];
            float new_re = old_re, new_im = old_im;
            if (dn > 0.0f) {
                new_re = __fdiv_rn(nr, dn);
                new_im = __fdiv_rn(ni, dn);
            }
            if ((k & 1) == 0) {
                new_re = __fmul_rn(__fadd_rn(new_re, old_re), 0.5f);
                new_im = __fmul_rn(__fadd_rn(new_im, old_im), 0.5f);
                const float dr = __fsub_rn(new_re, old_re), di = __fsub_rn(new_im, old_im);
                d_term[tid] = has_p ? ksp_norm2(make_float2(dr, di)) : 0.0f;
                n_term[tid] = has_p ? ksp_norm2(make_float2(new_re, new_im)) : 0.0f;
            }
            g_re[tid] = new_re;
            g_im[tid] = new_im;
            g_s[tid] = ksp_norm2(make_float2(new_re, new_im));
        }
        __syncthreads();
        if ((k & 1) == 0) {
            if (tid < blocks) {
                float d = 0.0f, m = 0.0f;
                const int end = min(n, (tid + 1) * SG_BLOCK);
                for (int i = tid * SG_BLOCK; i < end; i++) {
                    d = __fadd_rn(d, d_term[i]);
                    m = __fadd_rn(m, n_term[i]);
                }
                d_part[tid] = d;
                n_part[tid] = m;
            }
            __syncthreads();
            float d = d_part[0], m = n_part[0];
            for (int i = 1; i < blocks; i++) {
                d = __fadd_rn(d, d_part[i]);
                m = __fadd_rn(m, n_part[i]);
            }
            // (a NaN on either side: not converged. d_part is next written three barriers on)
            converged = d <= __fmul_rn(tol2, m);
        }
    }

    // ---- finish: referencing, corrections, NaN without data
    bool any_data = false;
    for (int i = 0; i < n; i++) any_data = any_data || has[i] != 0;
    bool referenced = false;
    float u_re = 1.0f, u_im = 0.0f;
    if (reference >= 0) {
        const float r_re = g_re[reference], r_im = g_im[reference];
        const float m = __builtin_sqrtf(ksp_norm2(make_float2(r_re, r_im)));
        referenced = has[reference] != 0 && m > 0.0f && m < __builtin_inff();
        if (referenced) {
            u_re = __fdiv_rn(r_re, m);
            u_im = __fdiv_rn(-r_im, m);
        }
    }
    if (tid < n) {
        float2 g = make_float2(g_re[tid], g_im[tid]);
        if (referenced) {
            g = ksp_cmul(g, make_float2(u_re, u_im));
            if (tid == reference) g.y = 0.0f;
        }
        if (corrections) g = ksp_creciprocal_or_nan(g);
        if (!has_p) g.x = g.y = __builtin_nanf("");
        gains[c * stride.gains + tid] = g;
    }
    if (tid == 0) {
        iterations[c] = k;
        status[c] = (uint8_t)((converged ? 0 : SG_NOT_CONVERGED) | (any_data ? 0 : SG_NO_DATA) |
                              (referenced ? 0 : SG_NOT_REFERENCED));
    }
}

extern "C" int ksp_solve_gains(int device, void *stream, const void *vis, const float *weights,
                               const uint8_t *flags, const int32_t *pairs, const void *initial,
                               void *gains, int32_t *iterations, uint8_t *status, int channels,
                               int baselines, int n_inputs, int vis_stride, int weights_stride,
                               int flags_stride, int pairs_stride, int initial_stride,
                               int gains_stride, int max_iterations, float tol2, int reference,
                               int mask, int corrections)
{
    const ksp_planes samples = {{"vis", vis, vis_stride, 8},
                                {"weights", weights, weights_stride, 4, true},
                                {"flags", flags, flags_stride, 1, true}};
    const ksp_plane p_initial = {"initial", initial, initial_stride, 8, true};
    const ksp_plane p_gains = {"gains", gains, gains_stride, 8};
    const ksp_planes tables = {{"pairs", pairs, pairs_stride, 4}, p_initial, p_gains};
    KSP_TRY(ksp_planes_given(samples));
    KSP_TRY(ksp_planes_given(tables));
    KSP_TRY(ksp_planes_given({{"iterations", iterations, 0, 4}, {"status", status, 0, 1}}));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_inputs >= 1 && n_inputs <= SG_MAX_INPUTS, "n_inputs must be 1..128");
    KSP_REQUIRE(max_iterations >= 1 && max_iterations <= SG_MAX_ITERATIONS,
                "max_iterations must be 1..1000");
    KSP_REQUIRE(tol2 >= 0.0f, "tol2 must be at least 0");
    KSP_REQUIRE(reference >= -1 && reference < n_inputs, "reference must be -1..n_inputs-1");
    KSP_REQUIRE(mask >= 0 && mask <= 255, "mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_TRY(ksp_planes_hold(samples, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold(tables, n_inputs, "n_inputs"));
    KSP_TRY(ksp_pairs_same_or_apart({p_initial, p_gains}, channels, n_inputs));

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const sg_strides stride = {vis_stride, weights_stride, flags_stride,
                               pairs_stride, initial_stride, gains_stride};
    const size_t lds_bytes = 4 * sg_lds_words(n_inputs);
    const int variant =
        (weights != nullptr ? 1 : 0) | (flags != nullptr ? 2 : 0) | (initial != nullptr ? 4 : 0);
    int rc = 0;
    ksp_dispatch_exact<0, 1, 2, 3, 4, 5, 6, 7>(variant, [&](auto V) {
        constexpr auto kernel =
            solve_gains_kernel<(V() & 1) != 0, (V() & 2) != 0, (V() & 4) != 0>;
        rc = ksp_lds_opt_in<kernel>(device, 4 * sg_lds_words(SG_MAX_INPUTS));
        if (rc != 0) return;
        hipLaunchKernelGGL(kernel, dim3((unsigned)channels), dim3(sg_threads(n_inputs)), lds_bytes,
                           s, (const float2 *)vis, weights, flags, (const int *)pairs,
                           (const float2 *)initial, (float2 *)gains, iterations, status, baselines,
                           n_inputs, stride, max_iterations, tol2, reference, (unsigned)mask,
                           corrections);
    });
    KSP_TRY(rc);
    KSP_LAUNCH_CHECK();
    return 0;
}
