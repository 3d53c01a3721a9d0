// masked_gaussian_filter (reference rfi/twodflag.py:254-400) on images [image][row][col],
// float32 or float64, any number of box passes.
//
// The reference carries one float64 running sum along every line it filters, so a line
// is sequential: a lane owns one line and runs the reference's loop in its order and
// precision. The parallelism is arrays (weight, masked data) x
// images x lines. A lane's padded line lives in the workspace interleaved
// ([position][lane]), so a wavefront's accesses to position i are contiguous.
//
//   mf_axis0   lanes (array, image, column): mask, filter along axis 0 (or copy when the
//              radius is 0) into W / O. Adjacent lanes are adjacent columns: image reads
//              and writes are contiguous by themselves.
//   mf_axis1   lanes (array, image, row): filters the rows of W / O in place. Rows enter
//              and leave a lane's line through an LDS tile of MF_THREADS rows x 128 bytes:
//              the workgroup loads and stores row segments (adjacent threads, adjacent
//              columns), the owning lane reads and writes its row of the tile. No global
//              access of this kernel has a wavefront's lanes one image row apart.
//   mf_finish  out = W == 0 ? NaN : O / W, elementwise into the caller's strided array.
#include <cmath>

#include "ksp_common.h"

#define MF_THREADS 256
#define MF_MAX_DIM 65536
#define MF_MAX_RADIUS 2047
#define MF_MAX_PASSES 8

namespace {

__device__ __forceinline__ float mf_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double mf_div(double a, double b) { return __ddiv_rn(a, b); }
template <class T>
__device__ __forceinline__ T mf_nan();
template <>
__device__ __forceinline__ float mf_nan<float>() { return __builtin_nanf(""); }
template <>
__device__ __forceinline__ double mf_nan<double>() { return __builtin_nan(""); }

// The K box passes of _box_gaussian_filter1d (twodflag.py:282-307) on one padded line
// P(0 .. n + r K), sums in float64, in the reference's order. Every pass keeps its
// support beyond the image. The caller guarantees tail >= start (K >= 2, or r <= n).
//
// The sum is one dependent chain, but its operands are not: within a pass every read is of
// the previous pass's value (P(i + 2r) is read at step i, before step i + 2r overwrites
// it), so the operands of MF_UNROLL steps are loaded together, the chain runs on
// registers and the results are stored together: one memory round trip per MF_UNROLL
// steps instead of one per step, the same additions in the same order.
#define MF_UNROLL 16

template <class T, class Acc>
__device__ __forceinline__ void mf_box_passes(const Acc &P, int n, int r, int K)
{
    const int padding = r * K, L = n + padding, r2 = 2 * r;
    int prev_start = padding;
    for (int p = 1; p <= K; ++p) {
        double s = 0.0;
        int start = padding - r2 * p;
        int stop = start + n + 2 * padding;
        start = max(start, 0);
        stop = min(stop, L);
        const int tail = min(stop, L - r2);
        const int head = min(start + r2, L);
        int i = prev_start;
        for (; i + MF_UNROLL <= head; i += MF_UNROLL) {
            T a[MF_UNROLL];
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) a[u] = P(i + u);
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) s += (double)a[u];
        }
        for (; i < head; ++i) s += (double)P(i);
        i = start;
        for (; i + MF_UNROLL <= tail; i += MF_UNROLL) {
            T a[MF_UNROLL], b[MF_UNROLL];
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) a[u] = P(i + u + r2);
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) b[u] = P(i + u);
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) {
                s += (double)a[u];
                const T prev = b[u];
                b[u] = (T)s;
                s -= (double)prev;
            }
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) P(i + u) = b[u];
        }
        for (; i < tail; ++i) {
            s += (double)P(i + r2);
            const T prev = P(i);
            P(i) = (T)s;
            s -= (double)prev;
        }
        for (; i + MF_UNROLL <= stop; i += MF_UNROLL) {
            T b[MF_UNROLL];
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) b[u] = P(i + u);
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) {
                const T prev = b[u];
                b[u] = (T)s;
                s -= (double)prev;
            }
#pragma unroll
            for (int u = 0; u < MF_UNROLL; ++u) P(i + u) = b[u];
        }
        for (; i < stop; ++i) {
            const T prev = P(i);
            P(i) = (T)s;
            s -= (double)prev;
        }
        prev_start = start;
    }
}

// Lanes: (array, image, column), array 0 = weight (not flagged), 1 = masked data.
// data / flags: caller's arrays (image stride si, row stride sr); W / O: [nb][rows][cols].
template <class T>
__global__ __launch_bounds__(MF_THREADS) void mf_axis0(
    const T *__restrict__ data, const uint8_t *__restrict__ flags, T *__restrict__ W,
    T *__restrict__ O, T *__restrict__ pad, int rows, int cols, int nb, size_t si, size_t sr,
    int r, int K, T div)
{
    const size_t per = (size_t)nb * cols, nl = 2 * per;
    const size_t lane = blockIdx.x * (size_t)MF_THREADS + threadIdx.x;
    if (lane >= nl) return;
    const int arr = lane >= per;
    const size_t rem = arr ? lane - per : lane;
    const size_t b = rem / cols, c = rem % cols;
    const size_t src = b * si + c;
    T *out = (arr ? O : W) + b * (size_t)rows * cols + c;
    auto value = [&](int t) -> T {
        const size_t i = src + (size_t)t * sr;
        return flags[i] ? (T)0 : (arr ? data[i] : (T)1);
    };
    if (r == 0) {
#pragma unroll 8
        for (int t = 0; t < rows; ++t) out[(size_t)t * cols] = value(t);
        return;
    }
    auto P = [&](int i) -> T & { return pad[(size_t)i * nl + lane]; };
    const int padding = r * K;
    for (int i = 0; i < padding; ++i) P(i) = (T)0;
#pragma unroll 8
    for (int t = 0; t < rows; ++t) P(padding + t) = value(t);
    mf_box_passes<T>(P, rows, r, K);
#pragma unroll 8
    for (int t = 0; t < rows; ++t) out[(size_t)t * cols] = mf_div(P(t), div);
}

// Lanes: (array, image, row); W and O are contiguous ([2][nb][rows][cols] from W), so line
// `lane` is the row at W + lane * cols. A tile holds TC = 128 / sizeof(T) columns of the
// workgroup's MF_THREADS rows, rows padded by one element against bank conflicts when
// the owning lanes read down a column of the tile.
template <class T>
__global__ __launch_bounds__(MF_THREADS) void mf_axis1(
    T *__restrict__ W, T *__restrict__ pad, int cols, size_t nl, int r, int K, T div)
{
    constexpr int TC = 128 / (int)sizeof(T);   // columns per tile
    constexpr int TR = MF_THREADS / TC;        // rows moved per step of the workgroup
    __shared__ T tile[MF_THREADS][TC + 1];
    const int tid = threadIdx.x;
    const size_t line0 = blockIdx.x * (size_t)MF_THREADS;
    const size_t lane = line0 + tid;
    const bool live = lane < nl;
    const int n_lines = (int)min((size_t)MF_THREADS, nl - line0);
    const int tc = tid % TC, tr = tid / TC;
    T *rows0 = W + line0 * cols;
    auto P = [&](int i) -> T & { return pad[(size_t)i * nl + lane]; };
    const int padding = r * K;
    if (live)
        for (int i = 0; i < padding; ++i) P(i) = (T)0;
    for (int c0 = 0; c0 < cols; c0 += TC) {
        const int w = min(TC, cols - c0);
        if (tc < w)
            for (int j = tr; j < n_lines; j += TR) tile[j][tc] = rows0[(size_t)j * cols + c0 + tc];
        __syncthreads();
        if (live)
            for (int c = 0; c < w; ++c) P(padding + c0 + c) = tile[tid][c];
        __syncthreads();
    }
    if (live) mf_box_passes<T>(P, cols, r, K);
    for (int c0 = 0; c0 < cols; c0 += TC) {
        const int w = min(TC, cols - c0);
        if (live)
            for (int c = 0; c < w; ++c) tile[tid][c] = mf_div(P(c0 + c), div);
        __syncthreads();
        if (tc < w)
            for (int j = tr; j < n_lines; j += TR) rows0[(size_t)j * cols + c0 + tc] = tile[j][tc];
        __syncthreads();
    }
}

template <class T>
__global__ __launch_bounds__(MF_THREADS) void mf_finish(
    const T *W, const T *O, T *out, int rows, int cols, int nb, size_t si, size_t sr)
{
    const size_t gid = blockIdx.x * (size_t)MF_THREADS + threadIdx.x;
    if (gid >= (size_t)nb * rows * cols) return;
    const size_t c = gid % cols, rest = gid / cols;
    const size_t t = rest % rows, b = rest / rows;
    const T w = W[gid];
    out[b * si + t * sr + c] = w == (T)0 ? mf_nan<T>() : mf_div(O[gid], w);
}

struct MfLayout {
    size_t W, O, pad, total;
};

size_t mf_align(size_t x) { return (x + 255) & ~(size_t)255; }

int mf_check(int rows, int cols, int batch, int r0, int r1, int passes, int itemsize)
{
    KSP_REQUIRE(rows >= 1 && rows <= MF_MAX_DIM, "rows outside 1..65536");
    KSP_REQUIRE(cols >= 1 && cols <= MF_MAX_DIM, "cols outside 1..65536");
    KSP_REQUIRE(batch >= 1, "batch < 1");
    KSP_REQUIRE(passes >= 1 && passes <= MF_MAX_PASSES, "passes outside 1..8");
    KSP_REQUIRE(r0 >= 0 && r0 <= MF_MAX_RADIUS, "radius of axis 0 outside 0..2047");
    KSP_REQUIRE(r1 >= 0 && r1 <= MF_MAX_RADIUS, "radius of axis 1 outside 0..2047");
    // one pass with a box radius beyond the line: the reference indexes before the start
    // of its padded line there
    KSP_REQUIRE(passes > 1 || (r0 <= rows && r1 <= cols),
                "passes = 1 needs radii within the image");
    KSP_REQUIRE(itemsize == 4 || itemsize == 8, "itemsize not 4 (float32) or 8 (float64)");
    return 0;
}

MfLayout mf_layout(int rows, int cols, int batch, int r0, int r1, int passes, int itemsize)
{
    MfLayout L;
    const size_t img = (size_t)rows * cols * batch * itemsize;
    // W and O back to back: mf_axis1 addresses both as one array of rows
    L.W = 0;
    L.O = img;
    L.pad = mf_align(2 * img);
    const size_t pad0 = r0 > 0 ? 2 * (size_t)batch * cols * (rows + (size_t)r0 * passes) : 0;
    const size_t pad1 = r1 > 0 ? 2 * (size_t)batch * rows * (cols + (size_t)r1 * passes) : 0;
    L.total = mf_align(L.pad + max(pad0, pad1) * itemsize);
    return L;
}

unsigned mf_blocks(size_t lanes) { return (unsigned)((lanes + MF_THREADS - 1) / MF_THREADS); }

template <class T>
void mf_run(hipStream_t s, const T *data, const uint8_t *flags, T *out, int rows, int cols,
            int nb, size_t si, size_t sr, int r0, int r1, int K, double d0, double d1, char *ws,
            const MfLayout &L)
{
    T *W = (T *)(ws + L.W), *O = (T *)(ws + L.O), *pad = (T *)(ws + L.pad);
    const size_t n0 = 2 * (size_t)nb * cols, n1 = 2 * (size_t)nb * rows;
    hipLaunchKernelGGL(mf_axis0<T>, dim3(mf_blocks(n0)), dim3(MF_THREADS), 0, s, data, flags, W, O,
                       pad, rows, cols, nb, si, sr, r0, K, (T)d0);
    if (r1 > 0)
        hipLaunchKernelGGL(mf_axis1<T>, dim3(mf_blocks(n1)), dim3(MF_THREADS), 0, s, W, pad, cols,
                           n1, r1, K, (T)d1);
    hipLaunchKernelGGL(mf_finish<T>, dim3(mf_blocks((size_t)nb * rows * cols)), dim3(MF_THREADS),
                       0, s, (const T *)W, (const T *)O, out, rows, cols, nb, si, sr);
}

}  // namespace

extern "C" int ksp_masked_filter_workspace(int rows, int cols, int batch, int r0, int r1,
                                           int passes, int itemsize, size_t *bytes)
{
    KSP_REQUIRE(bytes != nullptr, "NULL bytes");
    if (int rc = mf_check(rows, cols, batch, r0, r1, passes, itemsize)) return rc;
    *bytes = mf_layout(rows, cols, batch, r0, r1, passes, itemsize).total;
    return 0;
}

extern "C" int ksp_masked_filter(int device, void *stream, const void *data, const uint8_t *flags,
                                 void *out, int rows, int cols, int images,
                                 long long image_stride, long long row_stride, int image0,
                                 int batch, int r0, int r1, int passes, double divisor0,
                                 double divisor1, int itemsize, void *workspace,
                                 size_t workspace_bytes)
{
    KSP_REQUIRE(data != nullptr && flags != nullptr && out != nullptr && workspace != nullptr,
                "NULL buffer");
    if (int rc = mf_check(rows, cols, batch, r0, r1, passes, itemsize)) return rc;
    KSP_REQUIRE(images >= 1 && image0 >= 0 && (long long)image0 + batch <= images,
                "images [image0, image0 + batch) outside [0, images)");
    KSP_REQUIRE(row_stride >= cols && image_stride >= row_stride * rows, "strides too small");
    KSP_REQUIRE(image_stride <= (1LL << 40), "image stride beyond 2^40");
    KSP_REQUIRE(std::isfinite(divisor0) && divisor0 > 0 && std::isfinite(divisor1) && divisor1 > 0,
                "divisor not positive");
    const MfLayout L = mf_layout(rows, cols, batch, r0, r1, passes, itemsize);
    KSP_REQUIRE(workspace_bytes >= L.total, "workspace too small");
    KSP_REQUIRE(2 * (size_t)batch * max(rows, cols) <= 0x7fffffffull * MF_THREADS &&
                    (size_t)batch * rows * cols <= 0x7fffffffull * MF_THREADS,
                "batch too large for one launch");
    KSP_CHECK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const size_t si = (size_t)image_stride, sr = (size_t)row_stride, first = (size_t)image0 * si;
    if (itemsize == 4)
        mf_run<float>(s, (const float *)data + first, flags + first, (float *)out + first, rows,
                      cols, batch, si, sr, r0, r1, passes, divisor0, divisor1, (char *)workspace, L);
    else
        mf_run<double>(s, (const double *)data + first, flags + first, (double *)out + first, rows,
                       cols, batch, si, sr, r0, r1, passes, divisor0, divisor1, (char *)workspace, L);
    KSP_LAUNCH_CHECK();
    return 0;
}
