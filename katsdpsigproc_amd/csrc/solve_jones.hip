// solve_jones: per-antenna 2x2 Jones matrices solved from averaged visibilities, channel by
// channel, with the full-polarisation StEFCal step, in one launch (no reference counterpart).
// rfi/host.py SolveJonesHost is the definition; the kernel reproduces it bit for bit, under the
// rules of solve_gains.hip: every float step is one float32 operation (built with
// -ffp-contract=off and correctly rounded division and square root; steps written with
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn and the helpers of cal_math.h; square roots are
// __builtin_sqrtf), and every sum runs in blocks of SJ_BLOCK = 32 indices, sequential and
// ascending from +0 inside a block, the block sums added in ascending order.
//
// Input 2a + i is feed i of antenna a; row p of `jones` is z_p = (x, y) = (J[i][0], J[i][1]).
//   per channel, with A and W as in solve_gains and no entry within one antenna, z = initial or
//   the identity, for k = 1 .. max_iterations:
//     s00[q] = |x|^2;  s11[q] = |y|^2;  s01[q] = y conj(x)
//     num0[p] = sum_q A x;  num1[p] = sum_q A y               (A = A[p][q]; x, y of q)
//     h00[p] = sum_q W s00;  h11[p] = sum_q W s11;  h01[p] = sum_q (W s01.re, W s01.im)
//     det = h00 h11 - |h01|^2
//     det > 0:  c = num1 conj(h01);  e = num0 h01
//               new0 = ((num0.re h11 - c.re) / det, (num0.im h11 - c.im) / det)
//               new1 = ((num1.re h00 - e.re) / det, (num1.im h00 - e.im) / det)
//     else      new = z[p]
//     k odd:  z = new;    k even: z = (new + z) * 0.5, and stop when
//     sum_p (|dx|^2 + |dy|^2) <= tol2 * sum_p (|x|^2 + |y|^2)     (p over the inputs with data)
//   then referencing, corrections and NaN for the inputs without data.
//
// One workgroup per channel. The load phase is cal_triangle.h's. Iteration phase: thread (p, b)
// sums block b of row p: eight running sums, the element (p, q) from the triangle (conjugated
// below the diagonal, +0 on it) and the eight floats of input q as two 16-byte LDS broadcasts;
// thread p then adds the block sums, forms det and updates its row and its products (phase 1
// has finished: nobody reads the old row any more); on even k thread b sums block b of the two
// p-sums and every thread adds the block sums and takes the same decision. Two barriers per
// odd iteration, three per even one. The finish computes the reference's unitary factor in
// every thread from LDS.
//
// The workgroup has n * ceil(n / 32) threads rounded up to whole wavefronts, as solve_gains.
// No atomics, no workspace, no dependence on the order of workgroups. The sample arrays have
// any row stride; padding is neither read nor written. jones and initial are read and written
// 8 bytes at a time, so they need no more alignment than a complex64.
#include "cal_triangle.h"
#include "launch.h"

#define SJ_MAX_INPUTS 128
#define SJ_MAX_ITERATIONS 1000
#define SJ_BLOCK 32
#define SJ_MAX_BLOCKS (SJ_MAX_INPUTS / SJ_BLOCK)
#define SJ_NOT_CONVERGED 1
#define SJ_NO_DATA 2
#define SJ_NOT_REFERENCED 4
#define SJ_DET_NOT_POSITIVE 8

static int sj_blocks(int n_inputs) { return (n_inputs + SJ_BLOCK - 1) / SJ_BLOCK; }
static int sj_threads(int n_inputs) { return (n_inputs * sj_blocks(n_inputs) + 63) / 64 * 64; }
static int sj_pairs(int n_inputs) { return n_inputs * (n_inputs - 1) / 2; }
// Dynamic LDS in 4-byte words: eight floats per input (x, y, s00, s11, s01); eight block sums
// per (block, input); the two p-terms, the data mark and the "kept its row" mark per input; the
// block sums of the p-sums; three triangles
static size_t sj_lds_words(int n_inputs)
{
    return 8 * (size_t)n_inputs + 8 * (size_t)sj_blocks(n_inputs) * n_inputs +
           4 * (size_t)n_inputs + 2 * SJ_MAX_BLOCKS + 3 * (size_t)sj_pairs(n_inputs);
}

struct sj_strides {
    long long vis, weights, flags, pairs, initial, jones;
};

template <bool HAS_W, bool HAS_F, bool HAS_I>
__global__ __launch_bounds__(512) void solve_jones_kernel(
    const float2 *__restrict__ vis, const float *__restrict__ weights,
    const uint8_t *__restrict__ flags, const int *__restrict__ pairs, const float2 *initial,
    float2 *jones, int *__restrict__ iterations, uint8_t *__restrict__ status, int baselines, int n,
    sj_strides stride, int max_iterations, float tol2, int reference, unsigned mask,
    int corrections)
{
    extern __shared__ float4 sj_lds[];
    const int tid = threadIdx.x, threads = blockDim.x;
    const long long c = blockIdx.x;
    const int n_pairs = n * (n - 1) / 2;
    const int blocks = (n + SJ_BLOCK - 1) / SJ_BLOCK;
    float4 *zq = sj_lds;           // [q][2]: (x.re, x.im, y.re, y.im), (s00, s11, s01.re, s01.im)
    float4 *part = zq + 2 * n;     // [b][p][2]: (num0, num1), (h00, h11, h01)
    float *d_term = reinterpret_cast<float *>(part + 2 * blocks * n), *n_term = d_term + n;
    int *has = reinterpret_cast<int *>(n_term + n), *kept_row = has + n;
    float *d_part = reinterpret_cast<float *>(kept_row + n), *n_part = d_part + SJ_MAX_BLOCKS;
    float *a_re = n_part + SJ_MAX_BLOCKS, *a_im = a_re + n_pairs, *a_w = a_im + n_pairs;

    // ---- load: z and its products, the marks, then the triangle
    if (tid < n) {
        float2 x = make_float2((tid & 1) ? 0.0f : 1.0f, 0.0f);
        float2 y = make_float2((tid & 1) ? 1.0f : 0.0f, 0.0f);
        if (HAS_I) {
            x = initial[(c * stride.initial + tid) * 2];
            y = initial[(c * stride.initial + tid) * 2 + 1];
        }
        const float2 s01 = ksp_cmul_conj(y, x);
        zq[2 * tid] = make_float4(x.x, x.y, y.x, y.y);
        zq[2 * tid + 1] = make_float4(ksp_norm2(x), ksp_norm2(y), s01.x, s01.y);
        has[tid] = 0;
        kept_row[tid] = 0;
    }
    __syncthreads();
    ksp_triangle_load<HAS_W, HAS_F, true>(
        vis + c * stride.vis, HAS_W ? weights + c * stride.weights : nullptr,
        HAS_F ? flags + c * stride.flags : nullptr, pairs, stride.pairs, baselines, n, mask, a_re,
        a_im, a_w, has, tid, threads);
    __syncthreads();

    // ---- iterate
    const int b = tid / n, p = tid - b * n;  // thread (p, b); b >= blocks: only barriers
    const int q_begin = b * SJ_BLOCK, q_end = min(n, q_begin + SJ_BLOCK);
    const bool has_p = tid < n && has[tid] != 0;
    int k = 0;
    bool converged = false;
    while (k < max_iterations && !converged) {
        k++;
        if (b < blocks) {
            float2 num0 = make_float2(0.0f, 0.0f), num1 = num0, h01 = num0;
            float h00 = 0.0f, h11 = 0.0f;
#pragma unroll 4
            for (int q = q_begin; q < q_end; q++) {
                const int lo = min(p, q), hi = max(p, q);
                const bool off = p != q;
                const int e = off ? ksp_triangle_index(n, lo, hi) : 0;
                const float ar = off ? a_re[e] : 0.0f;
                float ai = off ? a_im[e] : 0.0f;
                const float w = off ? a_w[e] : 0.0f;
                if (p > q) ai = -ai;
                const float4 z = zq[2 * q], s = zq[2 * q + 1];
                const float2 a = make_float2(ar, ai);
                num0 = ksp_cadd(num0, ksp_cmul(a, make_float2(z.x, z.y)));
                num1 = ksp_cadd(num1, ksp_cmul(a, make_float2(z.z, z.w)));
                h00 = __fadd_rn(h00, __fmul_rn(w, s.x));
                h11 = __fadd_rn(h11, __fmul_rn(w, s.y));
                h01 = ksp_cadd(h01, make_float2(__fmul_rn(w, s.z), __fmul_rn(w, s.w)));
            }
            part[2 * (b * n + p)] = make_float4(num0.x, num0.y, num1.x, num1.y);
            part[2 * (b * n + p) + 1] = make_float4(h00, h11, h01.x, h01.y);
        }
        __syncthreads();
        if (tid < n) {
            float4 nu = part[2 * tid], h = part[2 * tid + 1];
            for (int i = 1; i < blocks; i++) {
                const float4 nu_i = part[2 * (i * n + tid)], h_i = part[2 * (i * n + tid) + 1];
                nu = make_float4(__fadd_rn(nu.x, nu_i.x), __fadd_rn(nu.y, nu_i.y),
                                 __fadd_rn(nu.z, nu_i.z), __fadd_rn(nu.w, nu_i.w));
                h = make_float4(__fadd_rn(h.x, h_i.x), __fadd_rn(h.y, h_i.y),
                                __fadd_rn(h.z, h_i.z), __fadd_rn(h.w, h_i.w));
            }
            const float2 num0 = make_float2(nu.x, nu.y), num1 = make_float2(nu.z, nu.w);
            const float h00 = h.x, h11 = h.y;
            const float2 h01 = make_float2(h.z, h.w);
            const float4 old = zq[2 * tid];
            float2 x = make_float2(old.x, old.y), y = make_float2(old.z, old.w);
            const float det = __fsub_rn(__fmul_rn(h00, h11), ksp_norm2(h01));
            if (det > 0.0f) {
                const float2 cc = ksp_cmul_conj(num1, h01), ee = ksp_cmul(num0, h01);
                x = make_float2(__fdiv_rn(__fsub_rn(__fmul_rn(num0.x, h11), cc.x), det),
                                __fdiv_rn(__fsub_rn(__fmul_rn(num0.y, h11), cc.y), det));
                y = make_float2(__fdiv_rn(__fsub_rn(__fmul_rn(num1.x, h00), ee.x), det),
                                __fdiv_rn(__fsub_rn(__fmul_rn(num1.y, h00), ee.y), det));
            }
            kept_row[tid] = has_p && !(det > 0.0f);
            if ((k & 1) == 0) {
                const float2 ox = make_float2(old.x, old.y), oy = make_float2(old.z, old.w);
                x = make_float2(__fmul_rn(__fadd_rn(x.x, ox.x), 0.5f),
                                __fmul_rn(__fadd_rn(x.y, ox.y), 0.5f));
                y = make_float2(__fmul_rn(__fadd_rn(y.x, oy.x), 0.5f),
                                __fmul_rn(__fadd_rn(y.y, oy.y), 0.5f));
                const float d = __fadd_rn(ksp_norm2(ksp_csub(x, ox)), ksp_norm2(ksp_csub(y, oy)));
                d_term[tid] = has_p ? d : 0.0f;
                n_term[tid] = has_p ? __fadd_rn(ksp_norm2(x), ksp_norm2(y)) : 0.0f;
            }
            const float2 s01 = ksp_cmul_conj(y, x);
            zq[2 * tid] = make_float4(x.x, x.y, y.x, y.y);
            zq[2 * tid + 1] = make_float4(ksp_norm2(x), ksp_norm2(y), s01.x, s01.y);
        }
        __syncthreads();
        if ((k & 1) == 0) {
            if (tid < blocks) {
                float d = 0.0f, m = 0.0f;
                const int end = min(n, (tid + 1) * SJ_BLOCK);
                for (int i = tid * SJ_BLOCK; i < end; i++) {
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
    bool any_data = false, any_kept = false;
    for (int i = 0; i < n; i++) {
        any_data = any_data || has[i] != 0;
        any_kept = any_kept || kept_row[i] != 0;
    }
    bool referenced = false;
    float2 u00 = make_float2(1.0f, 0.0f), u01 = make_float2(0.0f, 0.0f), u10 = u01, u11 = u00;
    if (reference >= 0) {
        const float4 r0 = zq[4 * reference], r1 = zq[4 * reference + 2];
        const float2 ra = make_float2(r0.x, r0.y), rb = make_float2(r0.z, r0.w);
        const float2 rc = make_float2(r1.x, r1.y), rd = make_float2(r1.z, r1.w);
        const float2 big_d = ksp_det2(ra, rb, rc, rd);
        const float m = __builtin_sqrtf(ksp_norm2(big_d));
        referenced = has[2 * reference] != 0 && has[2 * reference + 1] != 0 && m > 0.0f &&
                     m < __builtin_inff();
        if (referenced) {
            const float2 e = make_float2(__fdiv_rn(big_d.x, m), __fdiv_rn(big_d.y, m));
            const float2 b00 = ksp_cadd(ra, ksp_cmul_conj(e, rd));
            const float2 b01 = ksp_csub(rb, ksp_cmul_conj(e, rc));
            const float2 b10 = ksp_csub(rc, ksp_cmul_conj(e, rb));
            const float2 b11 = ksp_cadd(rd, ksp_cmul_conj(e, ra));
            const float t =
                __builtin_sqrtf(__builtin_sqrtf(ksp_norm2(ksp_det2(b00, b01, b10, b11))));
            u00 = make_float2(__fdiv_rn(b00.x, t), __fdiv_rn(b00.y, t));
            u01 = make_float2(__fdiv_rn(b01.x, t), __fdiv_rn(b01.y, t));
            u10 = make_float2(__fdiv_rn(b10.x, t), __fdiv_rn(b10.y, t));
            u11 = make_float2(__fdiv_rn(b11.x, t), __fdiv_rn(b11.y, t));
        }
    }
    if (tid < n) {
        // the two rows of this input's antenna, referenced; row `tid & 1` is this input's
        float2 rx[2], ry[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int r = (tid & ~1) + i;
            const float4 z = zq[2 * r];
            float2 x = make_float2(z.x, z.y), y = make_float2(z.z, z.w);
            if (referenced) {
                const float2 tx = ksp_row_dot_conj(x, y, u00, u01);
                const float2 ty = ksp_row_dot_conj(x, y, u10, u11);
                x = tx;
                y = ty;
                if (r == 2 * reference) x.y = 0.0f;
                if (r == 2 * reference + 1) y.y = 0.0f;
            }
            rx[i] = x;
            ry[i] = y;
        }
        const bool odd = (tid & 1) != 0;
        float2 x = odd ? rx[1] : rx[0], y = odd ? ry[1] : ry[0];
        const float nan32 = __builtin_nanf("");
        if (corrections) {
            const float2 inverse = ksp_creciprocal_or_nan(ksp_det2(rx[0], ry[0], rx[1], ry[1]));
            ksp_adj2_row_times(rx[0], ry[0], rx[1], ry[1], inverse, odd, x, y);
            // (a NaN `inverse` has left NaN in all four parts)
            if (has[tid & ~1] == 0 || has[tid | 1] == 0) x.x = x.y = y.x = y.y = nan32;
        } else if (!has_p) {
            x.x = x.y = y.x = y.y = nan32;
        }
        jones[(c * stride.jones + tid) * 2] = x;
        jones[(c * stride.jones + tid) * 2 + 1] = y;
    }
    if (tid == 0) {
        iterations[c] = k;
        status[c] = (uint8_t)((converged ? 0 : SJ_NOT_CONVERGED) | (any_data ? 0 : SJ_NO_DATA) |
                              (referenced ? 0 : SJ_NOT_REFERENCED) |
                              (any_kept ? SJ_DET_NOT_POSITIVE : 0));
    }
}

extern "C" int ksp_solve_jones(int device, void *stream, const void *vis, const float *weights,
                               const uint8_t *flags, const int32_t *pairs, const void *initial,
                               void *jones, int32_t *iterations, uint8_t *status, int channels,
                               int baselines, int n_inputs, int vis_stride, int weights_stride,
                               int flags_stride, int pairs_stride, int initial_stride,
                               int jones_stride, int max_iterations, float tol2, int reference,
                               int mask, int corrections)
{
    const ksp_planes samples = {{"vis", vis, vis_stride, 8},
                                {"weights", weights, weights_stride, 4, true},
                                {"flags", flags, flags_stride, 1, true}};
    // (an element of initial and of jones is a row of two complex64)
    const ksp_plane p_initial = {"initial", initial, initial_stride, 16, true};
    const ksp_plane p_jones = {"jones", jones, jones_stride, 16};
    const ksp_planes tables = {{"pairs", pairs, pairs_stride, 4}, p_initial, p_jones};
    KSP_TRY(ksp_planes_given(samples));
    KSP_TRY(ksp_planes_given(tables));
    KSP_TRY(ksp_planes_given({{"iterations", iterations, 0, 4}, {"status", status, 0, 1}}));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_inputs >= 2 && n_inputs <= SJ_MAX_INPUTS && n_inputs % 2 == 0,
                "n_inputs must be even and 2..128");
    KSP_REQUIRE(max_iterations >= 1 && max_iterations <= SJ_MAX_ITERATIONS,
                "max_iterations must be 1..1000");
    KSP_REQUIRE(tol2 >= 0.0f, "tol2 must be at least 0");
    KSP_REQUIRE(reference >= -1 && reference < n_inputs / 2,
                "reference must be -1..n_inputs/2-1");
    KSP_REQUIRE(mask >= 0 && mask <= 255, "mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_TRY(ksp_planes_hold(samples, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold(tables, n_inputs, "n_inputs"));
    KSP_TRY(ksp_pairs_same_or_apart({p_initial, p_jones}, channels, n_inputs));

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const sj_strides stride = {vis_stride, weights_stride, flags_stride,
                               pairs_stride, initial_stride, jones_stride};
    const size_t lds_bytes = 4 * sj_lds_words(n_inputs);
    const int variant =
        (weights != nullptr ? 1 : 0) | (flags != nullptr ? 2 : 0) | (initial != nullptr ? 4 : 0);
    int rc = 0;
    ksp_dispatch_exact<0, 1, 2, 3, 4, 5, 6, 7>(variant, [&](auto V) {
        constexpr auto kernel =
            solve_jones_kernel<(V() & 1) != 0, (V() & 2) != 0, (V() & 4) != 0>;
        rc = ksp_lds_opt_in<kernel>(device, 4 * sj_lds_words(SJ_MAX_INPUTS));
        if (rc != 0) return;
        hipLaunchKernelGGL(kernel, dim3((unsigned)channels), dim3(sj_threads(n_inputs)), lds_bytes,
                           s, (const float2 *)vis, weights, flags, (const int *)pairs,
                           (const float2 *)initial, (float2 *)jones, iterations, status, baselines,
                           n_inputs, stride, max_iterations, tol2, reference, (unsigned)mask,
                           corrections);
    });
    KSP_TRY(rc);
    KSP_LAUNCH_CHECK();
    return 0;
}
