// Fused single-pass RFI flagger for MI355X (gfx950).
//
// The reference runs five kernels (background -> transpose -> madnz_t ->
// threshold_sum -> transpose; reference rfi/device.py:1152-1164) and moves 31 bytes
// per sample through device memory. Here each visibility is read once (8 B) and each
// flag written once (1 B); everything in between stays on chip.
//
// Work decomposition ("strip" = FUSED_STRIP (4) adjacent baselines x all channels):
//   * one 256-thread workgroup (4 wavefronts) works on one strip; its LDS image is
//     ~76 KiB, so two workgroups share a CU and one's loads overlap the other's
//     arithmetic. strip_of() hands neighbouring strips to the same XCD at the same
//     time so that the 32-byte row segments of a 128-byte line meet in that XCD's L2;
//   * the strip is read as row segments (8 rows in flight per lane, double buffered),
//     turned into numpy's |z| and parked as float32 in LDS, transposed to
//     [baseline][channel];
//   * from then on wavefront w owns baseline w and lane l a run of R consecutive
//     channels: the sliding median (median_window.h), the MAD selection and
//     SumThreshold are wave-local, cross-lane traffic goes through shuffles/ballots;
//   * deviations are kept as float32 in registers (rounding is monotone, so ordering
//     decisions can be filtered on them); every value that decides a result - the
//     MAD's median candidates, window sums within their error bound of a threshold -
//     is recomputed exactly in float64 from the LDS amplitudes, because the host path
//     is float64 after the amplitude (reference rfi/host.py:148-163, 235-245) and the
//     flags must match it bit for bit.
//   * flags are zero-filled ahead of the kernel (a memset node, or a fill kernel when the
//     rows are not contiguous); the kernel only writes the (sparse) non-zero bytes.
//
// Roofline: HBM, 9 algorithmic bytes per sample (8 read + 1 written).
#include "flagger_fused_kernel.h"

// Events armed by ksp_flagger_fused_profile for the NEXT fused launch of this thread.
static thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;
// Kernels launched by this thread's last ksp_flagger_fused call (ksp_flagger_fused_last_path).
static thread_local int g_last_path = 0;

// Zero fill of `cols` bytes in each of `rows` rows that lie `stride` bytes apart. The rows are
// cut into the 16-byte aligned pieces of memory they touch, one piece per lane: a piece that
// lies wholly inside its row is one 16-byte store, the ragged first and last piece of a row are
// written byte by byte, and nothing between the rows is touched. `pieces` = pieces per row,
// enough for any alignment of a row's start: (cols + 15) / 16 + 1.
__global__ __launch_bounds__(256) void fused_zero_rows_kernel(uint8_t *__restrict__ base, int rows,
                                                              int cols, size_t stride, int pieces)
{
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = gid / (unsigned)pieces;
    if (row >= (size_t)rows) return;
    const int k = (int)(gid - row * (unsigned)pieces);
    const uintptr_t begin = (uintptr_t)base + row * stride, end = begin + (uintptr_t)cols;
    const uintptr_t piece = (begin & ~(uintptr_t)15) + 16 * (uintptr_t)k;
    if (piece >= end) return;
    if (piece >= begin && piece + 16 <= end) {
        *(uint4 *)piece = make_uint4(0u, 0u, 0u, 0u);
    } else {
        const uintptr_t lo = piece > begin ? piece : begin;
        const uintptr_t hi = piece + 16 < end ? piece + 16 : end;
        for (uintptr_t a = lo; a < hi; a++) *(uint8_t *)a = 0;
    }
}

hipError_t fused_zero_flags(const FusedParams &p, hipStream_t s)
{
    if (p.flags_stride == p.baselines)
        return hipMemsetAsync(p.flags, 0, (size_t)p.channels * p.baselines, s);
    const int pieces = (p.baselines + 15) / 16 + 1;
    const size_t lanes = (size_t)p.channels * pieces;
    hipLaunchKernelGGL(fused_zero_rows_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s,
                       p.flags, p.channels, p.baselines, (size_t)p.flags_stride, pieces);
    return hipGetLastError();
}

extern "C" int ksp_flagger_fused_profile(void *start_event, void *stop_event)
{
    KSP_REQUIRE((start_event == nullptr) == (stop_event == nullptr), "need both events or none");
    g_prof_start = (hipEvent_t)start_event;
    g_prof_stop = (hipEvent_t)stop_event;
    return 0;
}

extern "C" int ksp_flagger_fused_last_path(void) { return g_last_path; }

// ring kernel: 0 = by size, 1 = whenever it applies, -1 = never; per thread, as the launch is
static thread_local int g_ring_mode = 2;  // (2: not yet taken from the environment)
static int ring_mode()
{
    if (g_ring_mode == 2) {
        const char *e = getenv("KSP_FUSED_RING");
        g_ring_mode = e == nullptr ? 0 : (e[0] == '1' ? 1 : -1);
    }
    return g_ring_mode;
}
extern "C" int ksp_flagger_fused_ring_mode(int mode)
{
    const int before = ring_mode();
    if (mode >= -1 && mode <= 1) g_ring_mode = mode;
    return before;
}

extern "C" int ksp_flagger_fused_supported(int channels, int width, int n_windows)
{
    if (n_windows < 1 || n_windows > KSP_MAX_WINDOWS) return 0;
    if (channels > 4096) return n_windows <= 4 && ksp_fused_long_supported(channels, width);
    return channels >= 1 && width >= 3 && width <= 31 && (width & 1);
}

// The argument checks of ksp_flagger_fused; n_windows is normalised for the simple threshold.
static int check_fused_args(const void *vis, const uint8_t *in_flags, const uint8_t *flags,
                            const float *deviations, int channels, int baselines, int vis_stride,
                            int in_flags_stride, int flags_stride, int dev_stride, int width,
                            int flags_mode, int threshold_kind, const double *scales64,
                            int &n_windows)
{
    KSP_REQUIRE(vis != nullptr && flags != nullptr, "NULL buffer");
    KSP_REQUIRE(channels >= 1 && baselines >= 0, "bad shape");
    KSP_REQUIRE(vis_stride >= baselines && flags_stride >= baselines, "stride smaller than row");
    KSP_REQUIRE(deviations == nullptr || dev_stride >= baselines, "bad dev_stride");
    KSP_REQUIRE(flags_mode >= KSP_FLAGS_NONE && flags_mode <= KSP_FLAGS_FULL, "bad flags_mode");
    KSP_REQUIRE(flags_mode == KSP_FLAGS_NONE || in_flags != nullptr, "in_flags is NULL");
    KSP_REQUIRE(flags_mode != KSP_FLAGS_FULL || in_flags_stride >= baselines, "bad in_flags_stride");
    KSP_REQUIRE(threshold_kind == KSP_THRESHOLD_SIMPLE || threshold_kind == KSP_THRESHOLD_SUM,
                "bad threshold_kind");
    KSP_REQUIRE(threshold_kind == KSP_THRESHOLD_SIMPLE || scales64 != nullptr, "scales64 is NULL");
    if (threshold_kind == KSP_THRESHOLD_SIMPLE && n_windows < 1) n_windows = 1;
    if (!ksp_flagger_fused_supported(channels, width, n_windows)) {
        ksp_set_error("ksp_flagger_fused: unsupported configuration (channels=%d width=%d "
                      "n_windows=%d); use the per-stage kernels", channels, width, n_windows);
        return (int)hipErrorNotSupported;
    }
    // 16-byte loads of baseline pairs need even strides and an aligned base
    KSP_REQUIRE((vis_stride & 1) == 0, "vis_stride must be even");
    KSP_REQUIRE(((uintptr_t)vis & 15) == 0, "vis must be 16-byte aligned");
    return 0;
}

// The strip schedule of a launch over p.baselines baselines (fused_common.h, FusedParams):
// with a workspace for the counters, the last 1/16 of a large launch's strips are dynamic.
static void set_schedule(FusedParams &p, bool have_workspace)
{
    p.n_strips = ksp_divup(p.baselines, FUSED_STRIP);
    p.n_dyn = 0;
    if (have_workspace && p.n_strips >= 2048) p.n_dyn = (p.n_strips >> FUSED_DYN_SHIFT) & ~63;
    p.n_static = p.n_strips - p.n_dyn;
    p.dyn_blocks = p.n_dyn * FUSED_DYN_OVER / 4;
}

static FusedParams make_params(const void *vis, const uint8_t *in_flags, uint8_t *flags,
                               float *deviations, float *noise, int channels, int baselines,
                               int vis_stride, int in_flags_stride, int flags_stride,
                               int dev_stride, int is_amplitude, int flags_mode,
                               int threshold_kind, double n_sigma, const double *scales64,
                               int n_windows, int flag_value, void *workspace, int n_cu)
{
    FusedParams p = {};
    p.vis = vis;
    p.in_flags = in_flags;
    p.flags = flags;
    p.deviations = deviations;
    p.noise = noise;
    p.channels = channels;
    p.baselines = baselines;
    p.vis_stride = vis_stride;
    p.in_flags_stride = in_flags_stride;
    p.flags_stride = flags_stride;
    p.dev_stride = dev_stride;
    p.is_amplitude = is_amplitude;
    p.flags_mode = flags_mode;
    p.threshold_kind = threshold_kind;
    p.n_windows = n_windows;
    p.flag_value = flag_value;
    p.work = (unsigned *)workspace;
    set_schedule(p, workspace != nullptr);
    p.first_round = 2 * n_cu;
#ifdef KSP_DIAG
    const char *dbg = getenv("KSP_FUSED_DEBUG_STOP");
    p.debug_stop = dbg ? atoi(dbg) : 0;
#endif
    p.n_sigma = n_sigma;
    for (int k = 0; k < KSP_MAX_WINDOWS; k++)
        p.scales[k] = (scales64 != nullptr && k < n_windows) ? scales64[k] : 0.0;
    return p;
}

// Baselines [first, first + count) of a launch that the ring kernel accepts (complex
// visibilities, no input flags, no deviations), as a launch of its own on a static schedule.
static FusedParams columns(const FusedParams &p, int first, int count)
{
    FusedParams t = p;
    t.vis = (const float2 *)p.vis + first;
    t.flags = p.flags + first;
    if (p.noise != nullptr) t.noise = p.noise + first;
    t.baselines = count;
    set_schedule(t, false);
    return t;
}

// Which kernels take a launch: KSP_FUSED_PATH_* bits, the strip kernel's channels per lane (4,
// 16 or 64), and the baselines beyond the ring kernel's last whole strip of 8.
struct FusedPath {
    int bits, lanes, tail;
};

// `mode` is ksp_flagger_fused_ring_mode's (tests, diagnostics; initial value from
// KSP_FUSED_RING=1 / 0 in the environment): it forces the choice otherwise made by size.
// The persistent ring kernel takes the whole strips of 8 baselines of a 4096-channel
// launch without input flags; a ragged remainder (< 8 baselines) goes to the
// 4-baseline kernel.
// It pays from about 4 strips per workgroup on (measured, tools/time_ring_sizes.py: 0.089 ms
// against 0.065 at 4096 baselines, 0.133 = 0.132 at 8192, 0.218 against 0.236 at 16384,
// 0.384 against 0.431 at 32768).
static FusedPath choose_path(const FusedParams &p, int width, int n_cu, int mode)
{
    const bool want_ring = mode != 0 ? mode > 0 : p.baselines / 8 >= 4 * n_cu;
    if (want_ring && width == 13 && ksp_ring_supported(p, width)) {
        const int tail = p.baselines % 8;
        return {KSP_FUSED_PATH_RING | (tail != 0 ? KSP_FUSED_PATH_STRIP : 0), 64, tail};
    }
    if (p.channels > 4096) return {KSP_FUSED_PATH_LONG, 64, 0};
    // widths other than 13 and more than 4 SumThreshold windows: lanes always own 64 channels
    const bool wide = p.threshold_kind == KSP_THRESHOLD_SUM && p.n_windows > 4;
    if (width != 13 || wide || p.channels > 64 * 16) return {KSP_FUSED_PATH_STRIP, 64, 0};
    return {KSP_FUSED_PATH_STRIP, p.channels <= 64 * 4 ? 4 : 16, 0};
}

// The strip kernel for up to 4096 channels: width 13 is compiled here, the other widths in
// the flagger_fused_w*.hip files.
static int launch_strip(int lanes, int width, int device, hipStream_t s, const FusedParams &p,
                        hipEvent_t ev0, hipEvent_t ev1)
{
    if (width == 13) {
        if (lanes == 64) return launch_fused<64, 13>(device, s, p, ev0, ev1);
        if (lanes == 4) return launch_fused<4, 13>(device, s, p, ev0, ev1);
        return launch_fused<16, 13>(device, s, p, ev0, ev1);
    }
    int rc = 0;
    if (ksp_dispatch_exact<3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25, 27, 29, 31>(width, [&](auto W) {
            rc = ksp_fused_launch_width<W()>(device, s, p, ev0, ev1);
        }))
        return rc;
    ksp_set_error("fused flagger: width %d is not compiled here", width);
    return (int)hipErrorInvalidValue;
}

extern "C" int ksp_flagger_fused(int device, void *stream, const void *vis,
                                 const uint8_t *in_flags, uint8_t *flags, float *deviations,
                                 float *noise, int channels, int baselines, int vis_stride,
                                 int in_flags_stride, int flags_stride, int dev_stride, int width,
                                 int is_amplitude, int flags_mode, int threshold_kind,
                                 double n_sigma, const double *scales64, int n_windows,
                                 int flag_value, void *workspace)
{
    // profiling events are consumed by this call whatever its outcome
    const hipEvent_t ev0 = g_prof_start, ev1 = g_prof_stop;
    g_prof_start = g_prof_stop = nullptr;
    g_last_path = 0;
    int rc = check_fused_args(vis, in_flags, flags, deviations, channels, baselines, vis_stride,
                              in_flags_stride, flags_stride, dev_stride, width, flags_mode,
                              threshold_kind, scales64, n_windows);
    if (rc != 0 || baselines == 0) return rc;
    KSP_CHECK(hipSetDevice(device));
    static KspPerDevice<int> cus;
    int n_cu = cus.get(device);
    if (n_cu == 0) {
        KSP_CHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        cus.set(device, n_cu);
    }
    const FusedParams p = make_params(vis, in_flags, flags, deviations, noise, channels, baselines,
                                      vis_stride, in_flags_stride, flags_stride, dev_stride,
                                      is_amplitude, flags_mode, threshold_kind, n_sigma, scales64,
                                      n_windows, flag_value, workspace, n_cu);
    hipStream_t s = (hipStream_t)stream;
    const FusedPath path = choose_path(p, width, n_cu, ring_mode());
    if (path.bits & KSP_FUSED_PATH_RING) {
        // (Letting the ring kernel zero-fill `flags` itself -- write-through stores beside the
        // first strip's loads, a completion counter before the first flag byte -- was built
        // and measured: step time unchanged, 0.376 against 0.377 ms clean and 0.518 against
        // 0.519 with interference; the memset stays.)
        KSP_CHECK(fused_zero_flags(p, s));
        if (path.tail != 0) {
            const FusedParams t = columns(p, baselines - path.tail, path.tail);
            rc = launch_fused<64, 13>(device, s, t, nullptr, nullptr, false);
            if (rc != 0) return rc;
            g_last_path |= KSP_FUSED_PATH_STRIP;
        }
        g_last_path |= KSP_FUSED_PATH_RING;
        return ksp_ring_launch(width, device, s, p, n_cu, ev0, ev1);
    }
    g_last_path = path.bits;
    if (path.bits == KSP_FUSED_PATH_LONG) return ksp_fused_launch_long(device, s, p, ev0, ev1);
    return launch_strip(path.lanes, width, device, s, p, ev0, ev1);
}
