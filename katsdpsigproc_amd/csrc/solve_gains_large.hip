// solve_gains_large: what solve_gains computes, for up to 512 inputs (no reference counterpart).
// rfi/host.py SolveGainsLargeHost is the definition, SolveGainsHost with a larger limit; the
// kernel reproduces it bit for bit under the float discipline of solve_gains.hip: every float
// step is one float32 operation (-ffp-contract=off, __fmul_rn / __fadd_rn / __fsub_rn /
// __fdiv_rn, the one square root __builtin_sqrtf under correctly rounded division and square
// root), and every sum runs in the host's order: blocks of SGL_BLOCK = 32 indices, sequential
// and ascending from +0 inside a block, the block sums added in ascending order. The iteration,
// the sample-keeping rule, the rules for an entry of `pairs` (0, one beyond `baselines` and
// INT32_MIN form no address: baseline 0 is read instead and dropped), referencing, corrections,
// NaN for inputs without data and the status bits are those stated at the top of
// solve_gains.hip.
//
// A channel's matrix no longer fits LDS (12 n^2 bytes: 3 MiB at 512 inputs), so it lives in a
// work area in device memory that the caller supplies. A fixed grid of min(SGL_WORKGROUPS,
// channels) workgroups is launched; workgroup i solves channels i, i + G, i + 2 G, ... one
// after another in slot i of the work area: three planes (A.re, A.im, W) of n rows of
// ld = n rounded up to 32 floats, 12 n ld bytes. Plane element [q][p] holds element (p, q) of
// the host's matrices, stored in full: both halves, the lower one conjugated as the host
// stores it (kept ? -im : +0), +0 on the diagonal.
//
// Fill: thread p (one per input) writes column p of every row q, SGL_FILL rows per trip with
// their loads in flight together (first the entries of `pairs`, [min(p, q)][max(p, q)], then
// the samples they name), so a wavefront's stores run along a row. Every element of the n x n
// corner of the three planes is written for every channel before any is read: nothing depends
// on what the work area held before the launch or on the channel before. The columns n .. ld
// and whatever lies behind the slots are neither read nor written. Thread p alone decides
// whether input p has data (a kept sample in its row).
// Iterate: thread p owns row p of the host's matrices: it walks q ascending, reads plane
// element [q][p] (the lanes of a wavefront read consecutive addresses of one row), forms the
// 32-term block sums and their running total itself, SGL_UNROLL rows of loads in flight, with
// g and s broadcast from LDS; then it updates g[p] (after a barrier: nobody reads the old g any
// more). On even k thread b sums block b of the two p-sums and every thread adds the block sums
// and takes the same decision. Two barriers per odd iteration, three per even one, as in
// solve_gains. g, s, the data marks and the p-terms stay in LDS (12.4 KiB, static).
//
// The workgroup has n threads rounded up to whole wavefronts (192 at 129 .. 192 inputs, 512
// at 449 .. 512). No atomics; no workgroup waits for another or depends on the order in which
// they run; every loop is bounded by channels, n_inputs or max_iterations. The barriers order
// a workgroup's own stores to its slot before its own loads from it. The sample arrays have
// any row stride; padding is neither read nor written.
#include "cal_math.h"
#include "launch.h"

#define SGL_MAX_INPUTS 512
#define SGL_SMALL_INPUTS 128  // up to here ksp_solve_gains takes the call
#define SGL_MAX_ITERATIONS 1000
#define SGL_BLOCK 32
#define SGL_MAX_BLOCKS (SGL_MAX_INPUTS / SGL_BLOCK)
#define SGL_WORKGROUPS 256  // G: slots of the work area, and the most workgroups launched
#define SGL_FILL 8          // rows of the matrix a thread fills at once
#define SGL_UNROLL 16       // rows of the matrix a thread has in flight when it sums
#define SGL_NOT_CONVERGED 1
#define SGL_NO_DATA 2
#define SGL_NOT_REFERENCED 4

static int sgl_threads(int n_inputs) { return (n_inputs + 63) / 64 * 64; }
// Floats of a row of a plane: rows start on 128 bytes (given a work area that does)
static size_t sgl_ld(int n_inputs) { return ((size_t)n_inputs + 31) / 32 * 32; }
// Floats of a slot: three planes of n rows
static size_t sgl_slot_floats(int n_inputs) { return 3 * (size_t)n_inputs * sgl_ld(n_inputs); }

struct sgl_strides {
    long long vis, weights, flags, pairs, initial, gains;
};

template <bool HAS_W, bool HAS_F, bool HAS_I>
__global__ __launch_bounds__(512) void solve_gains_large_kernel(
    const float2 *__restrict__ vis, const float *__restrict__ weights,
    const uint8_t *__restrict__ flags, const int *__restrict__ pairs, const float2 *initial,
    float2 *gains, int *__restrict__ iterations, uint8_t *__restrict__ status, float *work,
    int channels, int baselines, int n, sgl_strides stride, int max_iterations, float tol2,
    int reference, unsigned mask, int corrections)
{
    __shared__ float g_re[SGL_MAX_INPUTS], g_im[SGL_MAX_INPUTS], g_s[SGL_MAX_INPUTS];
    __shared__ float d_term[SGL_MAX_INPUTS], n_term[SGL_MAX_INPUTS];
    __shared__ int has[SGL_MAX_INPUTS];
    __shared__ float d_part[SGL_MAX_BLOCKS], n_part[SGL_MAX_BLOCKS];
    const int tid = threadIdx.x;
    const int blocks = (n + SGL_BLOCK - 1) / SGL_BLOCK;
    const size_t ld = ((size_t)n + 31) / 32 * 32, plane = (size_t)n * ld;
    float *t_re = work + (size_t)blockIdx.x * 3 * plane, *t_im = t_re + plane, *t_w = t_im + plane;

    for (long long c = blockIdx.x; c < channels; c += gridDim.x) {
        // ---- fill: g, then column tid of the planes and this input's data mark
        bool has_p = false;
        if (tid < n) {
            float2 g0 = make_float2(1.0f, 0.0f);
            if (HAS_I) g0 = initial[c * stride.initial + tid];
            g_re[tid] = g0.x;
            g_im[tid] = g0.y;
            g_s[tid] = ksp_norm2(g0);
            const float2 *vis_row = vis + c * stride.vis;
            const float *weights_row = HAS_W ? weights + c * stride.weights : nullptr;
            const uint8_t *flags_row = HAS_F ? flags + c * stride.flags : nullptr;
            for (int q0 = 0; q0 < n; q0 += SGL_FILL) {
                // An entry that is no baseline (the diagonal and the rows past n among them)
                // reads baseline 0 instead (which exists) and its sample is dropped.
                int t[SGL_FILL];
#pragma unroll
                for (int u = 0; u < SGL_FILL; u++) {
                    const int q = q0 + u;
                    const int lo = min(tid, q), hi = max(tid, q);
                    t[u] = q < n && q != tid ? pairs[lo * stride.pairs + hi] : 0;
                }
                float2 v[SGL_FILL];
                float ws[SGL_FILL];
                unsigned f[SGL_FILL];
                bool valid[SGL_FILL];
#pragma unroll
                for (int u = 0; u < SGL_FILL; u++) {
                    valid[u] = t[u] > 0 ? t[u] <= baselines : (t[u] < 0 && t[u] >= -baselines);
                    const long long at = valid[u] ? (t[u] > 0 ? t[u] : -t[u]) - 1 : 0;
                    v[u] = vis_row[at];
                    ws[u] = HAS_W ? weights_row[at] : 1.0f;
                    f[u] = HAS_F ? flags_row[at] : 0u;
                }
#pragma unroll
                for (int u = 0; u < SGL_FILL; u++) {
                    const int q = q0 + u;
                    if (q >= n) continue;
                    const bool kept = valid[u] && !__builtin_isnan(v[u].x) &&
                                      !__builtin_isnan(v[u].y) && ws[u] > 0.0f && (f[u] & mask) == 0;
                    float re = 0.0f, im = 0.0f, w = 0.0f;
                    if (kept) {
                        re = __fmul_rn(ws[u], v[u].x);
                        im = __fmul_rn(ws[u], v[u].y);
                        if (t[u] < 0) im = -im;
                        if (tid > q) im = -im;  // (the lower half: the conjugate)
                        w = ws[u];
                        has_p = true;
                    }
                    const size_t e = q * ld + tid;
                    t_re[e] = re;
                    t_im[e] = im;
                    t_w[e] = w;
                }
            }
            has[tid] = has_p ? 1 : 0;
        }
        __syncthreads();

        // ---- iterate
        int k = 0;
        bool converged = false;
        while (k < max_iterations && !converged) {
            k++;
            float nr = 0.0f, ni = 0.0f, dn = 0.0f;  // the running totals of the block sums
            if (tid < n) {
                for (int q0 = 0; q0 < n; q0 += SGL_BLOCK) {
                    const int q1 = min(n, q0 + SGL_BLOCK);
                    float br = 0.0f, bi = 0.0f, bd = 0.0f;
                    for (int qu = q0; qu < q1; qu += SGL_UNROLL) {
                        // (a row past the block reads the block's last row and is dropped)
                        float ar[SGL_UNROLL], ai[SGL_UNROLL], w[SGL_UNROLL];
#pragma unroll
                        for (int u = 0; u < SGL_UNROLL; u++) {
                            const size_t e = min(qu + u, q1 - 1) * ld + tid;
                            ar[u] = t_re[e];
                            ai[u] = t_im[e];
                            w[u] = t_w[e];
                        }
#pragma unroll
                        for (int u = 0; u < SGL_UNROLL; u++) {
                            const int q = qu + u;
                            if (q >= q1) continue;
                            const float2 ag = ksp_cmul(make_float2(ar[u], ai[u]),
                                                       make_float2(g_re[q], g_im[q]));
                            br = __fadd_rn(br, ag.x);
                            bi = __fadd_rn(bi, ag.y);
                            bd = __fadd_rn(bd, __fmul_rn(w[u], g_s[q]));
                        }
                    }
                    nr = q0 == 0 ? br : __fadd_rn(nr, br);
                    ni = q0 == 0 ? bi : __fadd_rn(ni, bi);
                    dn = q0 == 0 ? bd : __fadd_rn(dn, bd);
                }
            }
            __syncthreads();
            if (tid < n) {
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
                    const int end = min(n, (tid + 1) * SGL_BLOCK);
                    for (int i = tid * SGL_BLOCK; i < end; i++) {
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
            bool any_data = false;
            for (int i = 0; i < n; i++) any_data = any_data || has[i] != 0;
            iterations[c] = k;
            status[c] = (uint8_t)((converged ? 0 : SGL_NOT_CONVERGED) |
                                  (any_data ? 0 : SGL_NO_DATA) |
                                  (referenced ? 0 : SGL_NOT_REFERENCED));
        }
        __syncthreads();  // (the next channel overwrites g and the data marks)
    }
}

// min(G, channels) slots of 12 n ld bytes, ld = n rounded up to 32: at 512 inputs 3 MiB a slot
// and at most 768 MiB, whatever `channels` is. Nothing up to 128 inputs, which ksp_solve_gains
// takes with the matrix in LDS.
extern "C" size_t ksp_solve_gains_large_work_bytes(int channels, int n_inputs)
{
    if (channels < 1 || n_inputs <= SGL_SMALL_INPUTS || n_inputs > SGL_MAX_INPUTS) return 0;
    const size_t slots = channels < SGL_WORKGROUPS ? channels : SGL_WORKGROUPS;
    return slots * sgl_slot_floats(n_inputs) * sizeof(float);
}

extern "C" int ksp_solve_gains_large(int device, void *stream, const void *vis,
                                     const float *weights, const uint8_t *flags,
                                     const int32_t *pairs, const void *initial, void *gains,
                                     int32_t *iterations, uint8_t *status, void *work_area,
                                     size_t work_bytes, int channels, int baselines, int n_inputs,
                                     int vis_stride, int weights_stride, int flags_stride,
                                     int pairs_stride, int initial_stride, int gains_stride,
                                     int max_iterations, float tol2, int reference, int mask,
                                     int corrections)
{
    const ksp_plane p_vis = {"vis", vis, vis_stride, 8};
    const ksp_plane p_weights = {"weights", weights, weights_stride, 4, true};
    const ksp_plane p_flags = {"flags", flags, flags_stride, 1, true};
    const ksp_plane p_pairs = {"pairs", pairs, pairs_stride, 4};
    const ksp_plane p_initial = {"initial", initial, initial_stride, 8, true};
    const ksp_plane p_gains = {"gains", gains, gains_stride, 8};
    const ksp_plane p_iterations = {"iterations", iterations, 0, 4};
    const ksp_plane p_status = {"status", status, 0, 1};
    const ksp_planes samples = {p_vis, p_weights, p_flags};
    const ksp_planes tables = {p_pairs, p_initial, p_gains};
    KSP_TRY(ksp_planes_given(samples));
    KSP_TRY(ksp_planes_given(tables));
    KSP_TRY(ksp_planes_given({p_iterations, p_status}));
    KSP_REQUIRE(channels >= 1, "channels must be at least 1");
    KSP_REQUIRE(baselines >= 1, "baselines must be at least 1");
    KSP_REQUIRE(n_inputs >= 1 && n_inputs <= SGL_MAX_INPUTS, "n_inputs must be 1..512");
    KSP_REQUIRE(max_iterations >= 1 && max_iterations <= SGL_MAX_ITERATIONS,
                "max_iterations must be 1..1000");
    KSP_REQUIRE(tol2 >= 0.0f, "tol2 must be at least 0");
    KSP_REQUIRE(reference >= -1 && reference < n_inputs, "reference must be -1..n_inputs-1");
    KSP_REQUIRE(mask >= 0 && mask <= 255, "mask must be 0..255");
    KSP_REQUIRE(corrections == 0 || corrections == 1, "corrections must be 0 or 1");
    KSP_TRY(ksp_planes_hold(samples, baselines, "baselines"));
    KSP_TRY(ksp_planes_hold(tables, n_inputs, "n_inputs"));
    KSP_TRY(ksp_pairs_same_or_apart({p_initial, p_gains}, channels, n_inputs));
    // Up to 128 inputs the matrix fits LDS: the kernel of solve_gains, and no work area
    if (n_inputs <= SGL_SMALL_INPUTS)
        return ksp_solve_gains(device, stream, vis, weights, flags, pairs, initial, gains,
                               iterations, status, channels, baselines, n_inputs, vis_stride,
                               weights_stride, flags_stride, pairs_stride, initial_stride,
                               gains_stride, max_iterations, tol2, reference, mask, corrections);
    KSP_REQUIRE(work_area != nullptr, "work_area is NULL");
    KSP_REQUIRE((uintptr_t)work_area % sizeof(float) == 0, "work_area is not 4-byte aligned");
    KSP_REQUIRE(work_bytes >= ksp_solve_gains_large_work_bytes(channels, n_inputs),
                "work_area is smaller than ksp_solve_gains_large_work_bytes");
    {
        // every byte the caller handed over as work area, against the data of every array
        const ksp_plane p_work = {"work_area", work_area, 0, 1};
        struct {
            const ksp_plane &plane;
            long long rows, cols;
        } const others[] = {{p_vis, channels, baselines},     {p_weights, channels, baselines},
                            {p_flags, channels, baselines},   {p_pairs, n_inputs, n_inputs},
                            {p_initial, channels, n_inputs},  {p_gains, channels, n_inputs},
                            {p_iterations, 1, channels},      {p_status, 1, channels}};
        for (const auto &o : others)
            if (o.plane.ptr != nullptr &&
                !ksp_planes_apart(p_work, 1, (long long)work_bytes, o.plane, o.rows, o.cols)) {
                ksp_set_error("invalid argument: work_area overlaps %s", o.plane.name);
                return (int)hipErrorInvalidValue;
            }
    }

    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const sgl_strides stride = {vis_stride, weights_stride, flags_stride,
                                pairs_stride, initial_stride, gains_stride};
    const int groups = channels < SGL_WORKGROUPS ? channels : SGL_WORKGROUPS;
    const int variant =
        (weights != nullptr ? 1 : 0) | (flags != nullptr ? 2 : 0) | (initial != nullptr ? 4 : 0);
    ksp_dispatch_exact<0, 1, 2, 3, 4, 5, 6, 7>(variant, [&](auto V) {
        constexpr auto kernel =
            solve_gains_large_kernel<(V() & 1) != 0, (V() & 2) != 0, (V() & 4) != 0>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(sgl_threads(n_inputs)), 0, s,
                           (const float2 *)vis, weights, flags, (const int *)pairs,
                           (const float2 *)initial, (float2 *)gains, iterations, status,
                           (float *)work_area, channels, baselines, n_inputs, stride,
                           max_iterations, tol2, reference, (unsigned)mask, corrections);
    });
    KSP_LAUNCH_CHECK();
    return 0;
}
