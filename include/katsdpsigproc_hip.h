/*
 * katsdpsigproc_hip.h -- C-ABI of the MI355X (gfx950) RFI-flagging library.
 *
 * The reference (ska-sa/katsdpsigproc) is pure Python: its device kernels are
 * Mako-templated C compiled at run time and launched through PyCUDA/PyOpenCL, so
 * it has no FFI of its own for this path. This header defines the boundary that
 * replaces that run-time compile-and-launch layer: every entry point names the
 * reference interface it stands in for (file:line below). All functions are
 * `extern "C"`, take plain pointers and sizes, return 0 on success or a non-zero
 * hipError_t, and record a message retrievable with ksp_last_error().
 *
 * Conventions (reference: SURVEY.md conventions; rfi/device.py docstrings):
 *   C = channels, B = baselines. Non-transposed arrays are [C][B] (baseline
 *   contiguous); `_t` arrays are [B][C]. Strides are in ELEMENTS of the array's
 *   dtype (the reference passes buffer.padded_shape[1], e.g. rfi/device.py:319).
 *   Device pointers must come from ksp_malloc (or any hipMalloc of the same
 *   process); kernels never allocate. `stream` is a hipStream_t (NULL = default).
 *   Launches are asynchronous and in-order on their stream, like the reference's
 *   command queues (doc/user/init.rst:37-39).
 */
#ifndef KATSDPSIGPROC_HIP_H
#define KATSDPSIGPROC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSP_ABI_VERSION 5

/* BackgroundFlags (reference: rfi/device.py:40-46) */
#define KSP_FLAGS_NONE 0
#define KSP_FLAGS_CHANNEL 1
#define KSP_FLAGS_FULL 2

/* threshold kinds for the fused flagger */
#define KSP_THRESHOLD_SIMPLE 0
#define KSP_THRESHOLD_SUM 1

#define KSP_MAX_WINDOWS 8

typedef struct ksp_device_props {
    char name[256];          /* AbstractDevice.name            (abc.py:105-108) */
    char arch[64];           /* gcnArchName, e.g. "gfx950:sramecc+:xnack-"      */
    int32_t compute_units;
    int32_t wavefront_size;  /* AbstractDevice.simd_group_size (abc.py:140-147) */
    int32_t max_threads_per_block;
    int32_t lds_bytes_per_block;
    int32_t clock_khz;
    int32_t driver_version;  /* AbstractDevice.driver_version  (abc.py:115-118) */
    int32_t runtime_version;
    int64_t total_memory;
} ksp_device_props;

/* ---- library / errors ---------------------------------------------------- */
int ksp_abi_version(void);
const char *ksp_last_error(void);

/* ---- devices (reference: cuda.py Device 87-160; abc.py:98-157) ------------ */
int ksp_device_count(int *count);
int ksp_device_get_props(int device, ksp_device_props *props);

/* ---- memory (reference: cuda.py Context.allocate_raw / allocate_pinned,
 *      cuda.py:189-222; abc.py:180-208) ------------------------------------- */
int ksp_malloc(int device, size_t bytes, void **ptr);
int ksp_free(int device, void *ptr);
int ksp_host_alloc(size_t bytes, void **ptr);
int ksp_host_free(void *ptr);

/* ---- streams and events (reference: cuda.py CommandQueue 249-479, Event 54-84;
 *      abc.py:71-95, 434-448) ------------------------------------------------ */
int ksp_stream_create(int device, void **stream);
int ksp_stream_destroy(int device, void *stream);
int ksp_stream_synchronize(int device, void *stream);
int ksp_event_create(int device, void **event);
/* An event that only orders work between streams of this device: no time stamp and no
 * system-scope fence (cache write-back + invalidate) when it is recorded. Not for
 * ksp_event_elapsed_ms, and not for handing results to the host. */
int ksp_event_create_ordering(int device, void **event);
int ksp_event_destroy(int device, void *event);
int ksp_event_record(int device, void *event, void *stream);
int ksp_event_synchronize(int device, void *event);
int ksp_event_elapsed_ms(int device, void *start, void *end, float *ms);
int ksp_stream_wait_event(int device, void *stream, void *event);

/* ---- copies (reference: abc.py:253-404; cuda.py:263-440). kind: 0 = host to
 *      device, 1 = device to host, 2 = device to device. The rect form copies
 *      shape[0] bytes x shape[1] x shape[2] with byte strides (strides[0] == 1),
 *      exactly the contract of enqueue_*_buffer_rect (abc.py:291-322). --------- */
int ksp_memcpy_async(int device, void *dst, const void *src, size_t bytes, int kind,
                     void *stream);
int ksp_memcpy_rect_async(int device, void *dst, size_t dst_origin, const size_t dst_strides[3],
                          const void *src, size_t src_origin, const size_t src_strides[3],
                          const size_t shape[3], int ndim, int kind, void *stream);
int ksp_memset_async(int device, void *ptr, int value, size_t bytes, void *stream);

/* ========================================================================== *
 *  Kernels. One launcher per reference kernel.
 *
 *  Sub-views. For every launcher, an array argument that comes with a row stride may
 *  be a sub-view of a larger array: a column block of a wider array, a buffer with a
 *  padding of its own, a pointer some elements into an allocation (one-dimensional
 *  arguments such as noise, mask or per-channel flags may start anywhere as well).
 *  With `cols` the extent of a row (baselines or channels, whichever is contiguous):
 *    - nothing outside [row * stride, row * stride + cols) of any row is written,
 *      zero fills included, and no input is written at all;
 *    - results do not depend on what lies outside those ranges;
 *    - alignment of pointers and strides affects speed only (16-byte loads and stores
 *      where every row allows them, element-wise access otherwise, same result),
 *      except where a launcher states a requirement: ksp_flagger_fused states one
 *      for `vis`.
 *  (ksp_twodflag, ksp_masked_filter and the FFT wrappers describe layouts of their own.)
 * ========================================================================== */

/* transpose (reference: transpose.mako:44-73; launch transpose.py:146-167).
 * dst[c][r] = src[r][c]; elem_size in {1,2,4,8,16} bytes. */
int ksp_transpose(int device, void *stream, void *dst, const void *src, int in_rows, int in_cols,
                  int out_stride, int in_stride, int elem_size);

/* percentile5_float (reference: percentile.mako:115-140; percentile.py:193-209).
 * Per row, over columns [first_col, first_col + n_cols): out[0..4][row] =
 * min, max, sorted[(n-1)/4], sorted[3(n-1)/4], sorted[(n-1)/2] of |in|.
 * is_amplitude: in is float32 (positive); else complex64 and |.| is numpy's abs.
 * n_cols 1..65536; more is rejected before any device call. Rows of 16385..65536 columns
 * run the radix-select kernel (csrc/percentile_long.h), exact for signed float32 values. */
int ksp_percentile5_float(int device, void *stream, const void *in, float *out, int rows,
                          int in_stride, int out_stride, int first_col, int n_cols,
                          int is_amplitude);

/* maskedsum_float (reference: maskedsum.mako:38-68; maskedsum.py:141-156).
 * out[col] = sum_row mask[row] * in[row][col]  (complex64 -> complex64), or
 * sum_row mask[row] * |in[row][col]| (-> float32) if use_amplitudes. */
int ksp_maskedsum_float(int device, void *stream, const void *in, const float *mask, void *out,
                        int in_stride, int n_rows, int n_cols, int use_amplitudes);

/* background_median_filter (reference: rfi/background_median_filter.mako:200-220;
 * launch rfi/device.py:311-325). in: [C][stride] complex64 or float32 amplitudes;
 * out: [C][stride] float32 deviations; flags: [C] (CHANNEL) or [C][flags_stride]
 * (FULL) uint8, any non-zero value masks the sample. width must be odd, 3..255 (checked
 * before any device call); 33..255 run the wide-window kernel (csrc/background_wide.h).
 * csplit: number of channel segments per baseline (the reference's tunable of the same
 * name, rfi/device.py:212-252), 0 = let the launcher choose. */
int ksp_background_median_filter(int device, void *stream, const void *in, float *out,
                                 const uint8_t *flags, int channels, int baselines, int stride,
                                 int flags_stride, int width, int is_amplitude, int flags_mode,
                                 int csplit);

/* How ksp_background_median_filter cuts the band for widths 3 .. 31 (no reference
 * counterpart: the tests use it to know which segment computed a channel). A wavefront
 * walks one segment of *seg_len channels for 64 adjacent baselines; segment i covers channels
 * [i * seg_len, min(channels, (i + 1) * seg_len)), and there are *n_segs of them. It is the
 * function the launcher itself calls. An empty band (channels or baselines 0) gives 0 and 0.
 * Host arithmetic only, no device call. Any other width is an error: the wide-window kernel
 * (33 .. 255) has a geometry of its own. */
int ksp_background_median_filter_geometry(int channels, int baselines, int width, int csplit,
                                          int *seg_len, int *n_segs);

/* madnz_t (reference: rfi/madnz_t.mako:72-87; launch rfi/device.py:594-607).
 * in: [B][stride] float32; noise[b] = float32(1.4826 * median(|x| : |x| > 0)): zeros and
 * NaN take no part, +-inf do; NaN if nothing is left.
 * channels 1..262144; more is rejected before any device call. */
int ksp_madnz_t(int device, void *stream, const float *in, float *noise, int channels,
                int baselines, int stride);

/* madnz (reference: rfi/madnz.mako:105-123; launch rfi/device.py:453-469).
 * Same statistic on channel-major data in: [C][stride]. */
int ksp_madnz(int device, void *stream, const float *in, float *noise, int channels,
              int baselines, int stride);

/* threshold_simple / threshold_simple_t (reference: rfi/threshold_simple.mako:27-40,
 * rfi/threshold_simple_t.mako:28-42; launch rfi/device.py:781-800).
 * flags = dev > n_sigma * noise[bl] ? flag_value : 0. rows x cols is the array
 * shape as stored: (C, B) if !transposed, (B, C) if transposed. */
int ksp_threshold_simple(int device, void *stream, const float *deviations, const float *noise,
                         uint8_t *flags, int rows, int cols, int stride, float n_sigma,
                         int flag_value, int transposed);

/* threshold_sum (reference: rfi/threshold_sum.mako:49-132; launch
 * rfi/device.py:968-987). deviations/flags: [B][stride]. Window k has size 2^k and
 * threshold float32(float32(n_sigma * noise[b]) * scales[k]) -- the float32 chain
 * numpy's host class follows when noise is float32 (rfi/host.py:235,252). Sums
 * are float64 over full windows only (rfi/host.py:239-242). scales is a HOST
 * pointer to n_windows floats (n_windows <= 8). vt: channels per thread (the
 * reference's tunable, rfi/device.py:868-887): 8, 16 or 32, 0 = let the launcher choose. */
int ksp_threshold_sum(int device, void *stream, const float *deviations, const float *noise,
                      uint8_t *flags, int channels, int baselines, int stride, float n_sigma,
                      const float *scales, int n_windows, int flag_value, int vt);

/* threshold_sum_cm: the same SumThreshold on channel-major data (no reference counterpart:
 * the reference transposes deviations to [B][C] and flags back). deviations/flags:
 * [C][stride], stride >= baselines, shared by both arrays; noise: [B]. Same thresholds,
 * float64 sums and full-window rule, so flags equal ksp_threshold_sum's on the transposed
 * array bit for bit. scales is a HOST pointer to n_windows floats (1..8). Every argument
 * is checked before any device call; the launcher picks the channel segmentation. */
int ksp_threshold_sum_cm(int device, void *stream, const float *deviations, const float *noise,
                         uint8_t *flags, int channels, int baselines, int stride, float n_sigma,
                         const float *scales, int n_windows, int flag_value);

/* Fused single-pass flagger: the MI355X-native form of FlaggerDevice
 * (reference: rfi/device.py:1062-1166 composes background -> [transpose] ->
 * noise_est -> threshold -> [transpose]). One launch reads vis [C][vis_stride]
 * once and writes flags [C][flags_stride]; everything after the float32
 * amplitude is float64, so flags are bit-identical to rfi.host.FlaggerHost
 * (rfi/host.py:270-273). deviations (float32, [C][dev_stride]) and noise
 * (float32 [B]) are optional outputs (NULL to skip). scales64 is a HOST pointer
 * to n_windows doubles (falloff^-k, rfi/host.py:215). workspace: NULL, or 64 bytes of
 * device memory owned by the caller, zeroed once when allocated and used by one
 * launch at a time (scheduling counters: with it the last strips of a large array are
 * handed to whichever XCD is free; the kernel leaves it zeroed again).
 * Alignment: vis must be 16-byte aligned and vis_stride even (both are checked before any
 * device call); every other array may be any sub-view. Only the `baselines` bytes of each
 * row of flags are cleared and written: one linear fill when flags_stride == baselines,
 * a row-wise fill kernel otherwise. */
int ksp_flagger_fused(int device, void *stream, const void *vis, const uint8_t *in_flags,
                      uint8_t *flags, float *deviations, float *noise, int channels,
                      int baselines, int vis_stride, int in_flags_stride, int flags_stride,
                      int dev_stride, int width, int is_amplitude, int flags_mode,
                      int threshold_kind, double n_sigma, const double *scales64, int n_windows,
                      int flag_value, void *workspace);

/* Arms two events (from ksp_event_create) for the calling thread's NEXT
 * ksp_flagger_fused call: they are recorded immediately before and after the flagger
 * kernel itself, excluding the zero-fill of flags that precedes it (the counterpart of
 * the reference's per-kernel profiling, abc.py:405-432 / TuningCommandQueue). Pass
 * NULL, NULL to disarm. */
int ksp_flagger_fused_profile(void *start_event, void *stop_event);

/* Returns 1 if ksp_flagger_fused supports this configuration (else callers fall
 * back to the kernel-per-stage sequence): up to 4096 channels with any odd width 3 .. 31
 * and 1 .. 8 SumThreshold windows (rfi/device.py:840-852 takes any n_windows); 4097 ..
 * 12288 channels with width 13 and at most 4 windows. */
int ksp_flagger_fused_supported(int channels, int width, int n_windows);

/* Which kernels the calling thread's LAST ksp_flagger_fused call launched (no reference
 * counterpart: the tests use it to prove which path they exercised): 0 none, or a sum of
 * STRIP = flagger_fused_kernel (strips of 4 baselines, up to 4096 channels),
 * LONG = flagger_long_kernel (4097-12288 channels),
 * RING = flagger_ring_kernel (persistent, strips of 8 baselines, 4096 channels, complex input
 *     without input flags, no deviations output, at most 4 windows; chosen from about 4
 *     strips per compute unit on, see ksp_flagger_fused_ring_mode); RING | STRIP = ring kernel
 *     plus the 4-baseline kernel for a remainder of fewer than 8 baselines. */
#define KSP_FUSED_PATH_STRIP 1
#define KSP_FUSED_PATH_LONG 2
#define KSP_FUSED_PATH_RING 4
int ksp_flagger_fused_last_path(void);

/* Which launches of the calling thread take the persistent ring kernel where it applies
 * (no reference counterpart; tests and diagnostics): 0 = those with at least 4 strips of 8
 * baselines per compute unit (the default), 1 = all, -1 = none. The initial value comes from
 * KSP_FUSED_RING=1 / 0 in the environment if set. Returns the previous mode; any other
 * argument only queries. */
int ksp_flagger_fused_ring_mode(int mode);

/* Self-tests of the arithmetic building blocks (no reference counterpart; they exist
 * so that the test-suite can pin device arithmetic against IEEE / numpy results).
 * ksp_selftest_sqrt12: out[i] = the kernels' square root of the float32 with bit
 *   pattern 0x3f800000 + i (i.e. every float32 from 1.0 upwards; n <= 2^23 + 1 covers
 *   [1, 2]), to be compared with a correctly rounded sqrt.
 * ksp_selftest_abs: out[i] = the kernels' |re[i] + j im[i]| (numpy's complex64 abs,
 *   rfi/host.py:137). All pointers are device pointers. */
int ksp_selftest_sqrt12(int device, void *stream, float *out, int n);
int ksp_selftest_abs(int device, void *stream, const float *re, const float *im, float *out,
                     int n);

/* Self-tests of the rank / reduction library (csrc/rank.h, bitplane.h), the counterpart
 * of the reference's test kernels test/test_rank.mako:37-113 driven by
 * test/test_rank.py:67-213. One 256-thread workgroup each; device pointers.
 * ksp_selftest_rank: out[q] = number of the n <= 2048 non-negative floats in data that
 *   are strictly below q, for 0 <= q < m (rank.mako:31-105 `rank`; NaN never counts).
 * ksp_selftest_minmax: out[0] / out[1] = smallest / largest non-NaN value of the
 *   n <= 2048 floats, NaN if all are NaN (rank.mako:57-84).
 * ksp_selftest_median_non_zero: median of the non-zero values of n <= 16384
 *   non-negative floats (float32 mean of the middle two for an even count,
 *   rank.mako:253-267): out[0] by the workgroup search, out[1] by the wavefront
 *   bit-plane search when n <= 4096 (else the workgroup search again). */
int ksp_selftest_rank(int device, void *stream, const float *data, int *out, int n, int m);
int ksp_selftest_minmax(int device, void *stream, const float *data, float *out, int n);
int ksp_selftest_median_non_zero(int device, void *stream, const float *data, float *out,
                                 int n);

/* ---- run-time compilation and generic launch (reference abc.py:160-245 `compile`,
 * 406-432 `enqueue_kernel`; cuda.py:182-187, 442-459) ----
 * ksp_rtc_compile: compile HIP `source` with hiprtc for the device's architecture
 *   (options: n_options strings such as "-DNAME=1", "-I/dir") and load it; *module_out
 *   receives a module handle. The compiler's log (warnings, or the errors on failure)
 *   is copied to `log` (NUL-terminated, at most log_capacity bytes; may be NULL).
 * ksp_module_get_function: kernel `name` (an extern "C" __global__ function) of a module.
 * ksp_launch_function: launch with grid/block given as 3 unsigned each (in workgroups /
 *   threads) and kernel_params = array of pointers to the argument values, in order.
 * ksp_module_unload: free the module. */
int ksp_rtc_compile(int device, const char *source, const char *const *options, int n_options,
                    void **module_out, char *log, size_t log_capacity);
int ksp_module_get_function(int device, void *module, const char *name, void **function_out);
int ksp_module_unload(int device, void *module);
int ksp_launch_function(int device, void *stream, void *function, const unsigned *grid,
                        const unsigned *block, unsigned shared_bytes, void **kernel_params);

/* ---- FFT over hipFFT (reference fft.py:64-202 binds cuFFT the same way) ----
 * Transform types (the values hipFFT and cuFFT share). */
#define KSP_FFT_R2C 0x2a
#define KSP_FFT_C2R 0x2c
#define KSP_FFT_C2C 0x29
#define KSP_FFT_D2Z 0x6a
#define KSP_FFT_Z2D 0x6c
#define KSP_FFT_Z2Z 0x69
/* ksp_fft_plan_create: batched plan of `rank` (1..3) dimensions n[], unit strides, with
 *   padded (embedding) shapes and batch distances in elements on both sides
 *   (hipfftMakePlanMany64; reference fft.py:304-323). Automatic work-area allocation is
 *   off: *work_size bytes must be supplied to ksp_fft_exec.
 * ksp_fft_exec: run the plan on `stream`; inverse selects the direction of C2C / Z2Z
 *   (real transforms have only one). Unnormalised, like the reference. */
int ksp_fft_plan_create(int device, int rank, const long long *n, const long long *inembed,
                        long long idist, const long long *onembed, long long odist, int type,
                        long long batch, void **plan_out, size_t *work_size);
int ksp_fft_plan_destroy(int device, void *plan);
int ksp_fft_exec(int device, void *stream, void *plan, int type, void *src, void *dest,
                 void *work_area, int inverse);

/* ---- Two-dimensional SumThreshold flagger (reference rfi/twodflag.py:236-482) ----
 * Parameters as the reference's SumThresholdFlagger._get_flags hands them to
 * _get_flags_impl, already conditioned on the host: windows clipped (and, for frequency,
 * scaled and made unique), chunk ends from numpy.linspace, spike_width_freq divided by
 * average_freq. tf_* = rho ** log2(window); threshold_scale = outlier_nsigma * MAD_NORMAL;
 * reject_scale = MAD_NORMAL * background_reject (all float64, as numba computes them).
 * Limits: n_time 1..KSP_TDF_MAX_TIME, n_freq 1..KSP_TDF_MAX_FREQ, 1..32 windows per axis,
 * 1..KSP_TDF_MAX_CHUNKS frequency chunks, background_iterations 0..64, box-filter radii
 * up to KSP_TDF_MAX_RADIUS. */
#define KSP_TDF_MAX_TIME 4096
#define KSP_TDF_MAX_FREQ 65536
#define KSP_TDF_MAX_WINDOWS 32
#define KSP_TDF_MAX_CHUNKS 512
#define KSP_TDF_MAX_RADIUS 2047
typedef struct ksp_twodflag_params {
    int n_time, n_freq, average_freq, is_amplitude;
    int n_windows_time, n_windows_freq;
    int windows_time[KSP_TDF_MAX_WINDOWS], windows_freq[KSP_TDF_MAX_WINDOWS];
    double tf_time[KSP_TDF_MAX_WINDOWS], tf_freq[KSP_TDF_MAX_WINDOWS];
    int n_chunks;
    int chunk_ends[KSP_TDF_MAX_CHUNKS + 1];
    int background_iterations, time_extend, freq_extend;
    double spike_width_time, spike_width_freq;
    double threshold_scale, reject_scale, flag_all_time_frac, flag_all_freq_frac;
} ksp_twodflag_params;
/* ksp_twodflag_workspace: bytes of device workspace for batches of `batch` baselines.
 * ksp_twodflag: flags for baselines [bl0, bl0 + batch) of data[n_time][n_freq][n_bl]
 *   (complex64, or float32 if is_amplitude), in_flags and out_flags uint8 of the same
 *   layout; stride_t and stride_f are the element strides of the time and channel axes
 *   (baselines contiguous). out = reference get_flags(...) for those baselines. Every
 *   argument is checked before any device call. */
int ksp_twodflag_workspace(const ksp_twodflag_params *params, int batch, size_t *bytes);
/* Byte offsets within the workspace of the temporaries a ksp_twodflag call leaves there.
 * After the call returns (and its stream has drained), they hold the stages of that call's
 * batch, baseline-major: B = batch, T = n_time, A = averaged channels, F = n_freq;
 * float32 where named so, else uint8 0/1.
 *   spec_flags [B][A]            median spectrum flags (no unflagged time)
 *   spec_background [B][A]       float32, background of the median spectrum
 *   spec_residual [B][A]         float32, median spectrum - its background
 *   spec_st [B][A]               SumThreshold flags of the spectrum
 *   flags [B][T][A]              averaged input flags | spec_st
 *   background [B][T][A]         float32, 2-D background
 *   residual [B][T][A]           float32, averaged data - 2-D background
 *   time_flags, freq_flags [B][T][A]   SumThreshold along time / along frequency
 *   combined [B][T][A]           spec_st | time | frequency flags, smeared in time
 *   row_flags [B][T][F]          combined, un-averaged and smeared in frequency
 *   row_all [B][T], col_all [B][F]     whole-time / whole-channel flags
 * ksp_twodflag_layout checks its arguments as ksp_twodflag_workspace does; host only. */
typedef struct ksp_twodflag_offsets {
    size_t spec_flags, spec_background, spec_residual, spec_st;
    size_t flags, background, residual, time_flags, freq_flags, combined;
    size_t row_flags, row_all, col_all;
} ksp_twodflag_offsets;
int ksp_twodflag_layout(const ksp_twodflag_params *params, int batch, ksp_twodflag_offsets *out);
int ksp_twodflag(int device, void *stream, const void *data, const uint8_t *in_flags,
                 uint8_t *out_flags, int n_bl, long long stride_t, long long stride_f, int bl0,
                 int batch, const ksp_twodflag_params *params, void *workspace,
                 size_t workspace_bytes);

/* flag_count (no reference counterpart: the reference's callers count on a host copy).
 * flags: [rows][stride] uint8. For each of the n_masks (1..8) non-zero masks,
 * row_counts[m * row_counts_stride + r] = number of columns c with flags[r][c] & masks[m] != 0,
 * col_counts[m * col_counts_stride + c] = number of rows r with flags[r][c] & masks[m] != 0:
 * a sample counts at most once per mask, masks may overlap. One launch reads every flag
 * byte once and produces both. accumulate == 0: both outputs are overwritten (their zero
 * fill is enqueued on the stream by the launcher); otherwise the counts are added to what
 * the outputs hold, modulo 2^32. Bytes between cols and stride are never counted, counters
 * between rows / cols and their stride never written. masks is a HOST pointer. flags or
 * stride that are not multiples of 16 take a slower, byte-wise path with the same result.
 * Every argument is checked before any device call. */
int ksp_flag_count(int device, void *stream, const uint8_t *flags, uint32_t *row_counts,
                   uint32_t *col_counts, int rows, int cols, int stride, int row_counts_stride,
                   int col_counts_stride, const uint8_t *masks, int n_masks, int accumulate);

/* average (no reference counterpart: the reference's callers average in their own code).
 * Flag-aware averaging over dumps and over groups of channels, bit for bit what
 * rfi/host.py AveragerHost computes; all arithmetic is float32, one rounding per step.
 * Every array is [channels][stride] with baselines contiguous and its own row stride, in
 * elements (vis arrays: complex64 elements). Elements between baselines and a stride are
 * neither read nor written. Pointers and strides that make every row start a multiple of
 * 16 bytes take 16-byte loads and stores; anything else a slower element-wise path with
 * the same result. Every argument is checked before any device call.
 *
 * ksp_average_accumulate adds one dump to the accumulators, per sample:
 *   f = flags | input_flags;  we = f != 0 ? w * 2^-64 : w;
 *   acc_vis.re += we * vis.re;  acc_vis.im += we * vis.im  (a multiply, then an add);
 *   acc_weights += we;  acc_flags |= f.
 * weights may be NULL (w = 1; weights_stride is then ignored). input_flags_mode: 0 none
 * (input_flags must be NULL), 1 one byte per channel (uint8 [channels]), 2 one byte per
 * sample ([channels][input_flags_stride]); the stride is ignored unless the mode is 2.
 * The caller zeroes the accumulators before the first dump.
 *
 * ksp_average_finalise writes channels / channel_factor rows of out_vis, out_weights and
 * out_flags. Per output: re, im, w start at +0 and fl at 0; rows r * channel_factor + k,
 * k = 0 .. channel_factor - 1, of the accumulators are added (ORed) in that order;
 * if w < 2^-32 ("every contribution was flagged") re, im and w are multiplied by 2^64;
 * out_vis = w > 0 ? (re / w, im / w) : (0, 0) with two correctly rounded divisions;
 * out_weights = w; out_flags = fl if every contribution was flagged, else 0.
 * clear != 0: the accumulator elements that were read are set to zero in the same pass.
 *
 * ksp_average_accumulate_block adds n_dumps dumps (1..8) in one launch: for every sample
 * the steps of ksp_average_accumulate on dump 0, then on dump 1, and so on, so the result is
 * bit for bit that of n_dumps calls in that order, while the accumulators are read and
 * written once. vis, flags, weights and input_flags are host arrays of n_dumps device
 * pointers (read during the call); the dumps are read-only and may repeat. weights as a
 * whole may be NULL, input_flags as a whole is NULL exactly when the mode is 0, and no entry
 * of a list that is given may be NULL. One row stride per kind serves every dump. One
 * pointer of one dump that is not 16-byte aligned sends the whole call down the element
 * path. */
int ksp_average_accumulate(int device, void *stream, const void *vis, const uint8_t *flags,
                           const float *weights, const uint8_t *input_flags,
                           int input_flags_mode, void *acc_vis, float *acc_weights,
                           uint8_t *acc_flags, int channels, int baselines, int vis_stride,
                           int flags_stride, int weights_stride, int input_flags_stride,
                           int acc_vis_stride, int acc_weights_stride, int acc_flags_stride);
int ksp_average_accumulate_block(int device, void *stream, int n_dumps, const void *const *vis,
                                 const uint8_t *const *flags, const float *const *weights,
                                 const uint8_t *const *input_flags, int input_flags_mode,
                                 void *acc_vis, float *acc_weights, uint8_t *acc_flags,
                                 int channels, int baselines, int vis_stride, int flags_stride,
                                 int weights_stride, int input_flags_stride, int acc_vis_stride,
                                 int acc_weights_stride, int acc_flags_stride);
int ksp_average_finalise(int device, void *stream, void *acc_vis, float *acc_weights,
                         uint8_t *acc_flags, void *out_vis, float *out_weights,
                         uint8_t *out_flags, int channels, int baselines, int channel_factor,
                         int clear, int acc_vis_stride, int acc_weights_stride,
                         int acc_flags_stride, int out_vis_stride, int out_weights_stride,
                         int out_flags_stride);

/* sir: the scale-invariant rank operator along one axis of flags [rows][stride] uint8, in
 * place (no reference counterpart; bit for bit what rfi/host.py ScaleInvariantRankHost
 * computes). axis 0: a line is a column, `cols` lines of `rows` samples (the flagger's
 * channels x baselines output); axis 1: a line is a row, `rows` lines of `cols` samples (the
 * baselines x channels layout). A line has 1 .. 262144 samples. A sample is flagged when
 * flags & mask != 0. With psi = eta_q for a flagged sample and eta_q - 4096 for any other, and
 * M(j) the sum of psi over the first j samples of the line (int32), sample x is in the result
 * iff max over b in (x, n] of M(b) >= min over a in [0, x] of M(a): x lies in an interval
 * [a, b) with 4096 * #flagged(a, b) >= (4096 - eta_q) * (b - a). Every sample of the result
 * gets flags |= flag_value; every other bit of every byte is kept. The result contains the
 * input; eta_q = 0 (0 .. 4096 allowed) adds nothing, 4096 flags everything. mask and
 * flag_value are 1 .. 255 and may overlap. Row offsets are 64-bit; bytes between cols and
 * stride are never read and never written. flags or stride that are odd (axis 0, also an odd
 * cols) or not multiples of 16 (axis 1) take a slower, byte-wise path with the same result.
 * No workspace. Every argument is checked before any device call. */
int ksp_sir(int device, void *stream, uint8_t *flags, int rows, int cols, int stride, int axis,
            int eta_q, int mask, int flag_value);

/* prepare: a correlator's integer dump as the inputs of the flagging chain, in one launch (no
 * reference counterpart; bit for bit what rfi/host.py PrepareHost computes; every float step
 * is one float32 operation, rounded once).
 * vis_in: [channels][vis_in_stride] pairs (re, im) of int32, of which in_baselines are data.
 * source: int32 [baselines]; auto_source: int32 [baselines][2], contiguous. vis: complex64,
 * input_flags: uint8, weights: float32, each [channels][its stride], baselines contiguous.
 * Strides are in elements of their array (pairs for vis_in, complex numbers for vis).
 * Per channel c and output baseline j, with s = source[j]:
 *   lost = s outside 0 .. in_baselines - 1, or vis_in[c][s].re == -2^31 (a sample that was
 *          never received; vis_in[c][s].im == -2^31 alone is data);
 *   vis = lost ? (0, 0) : (float(re) * scale, float(im) * scale);
 *   input_flags = (channel_flags ? channel_flags[c] : 0) | (lost ? lost_flag : 0);
 *   power(k) = k inside 0 .. in_baselines - 1 and vis_in[c][k].re != -2^31
 *              ? float(vis_in[c][k].re) * scale : 0;
 *   pa = power(auto_source[j][0]), pb = power(auto_source[j][1]), d = pa * pb;
 *   weights = pa > 0 && pb > 0 && d > 0 ? weight_scale / d : 0 (correctly rounded).
 * Any int32 is allowed in source and auto_source: an index outside the range is never used
 * to form an address. channel_flags (uint8 [channels]) may be NULL; auto_source and weights
 * are both NULL (no weights; weights_stride and weight_scale are then ignored) or both given.
 * scale and weight_scale are finite and positive, lost_flag is 1 .. 255. Elements between
 * baselines and a stride are never written, elements between in_baselines and vis_in_stride
 * never read. 16-byte stores need vis, input_flags, weights, source and auto_source and every
 * row start to be multiples of 16 bytes and vis_in a multiple of 8; anything else takes a
 * slower element-wise path with the same result. Every argument is checked before any device
 * call. */
int ksp_prepare(int device, void *stream, const int32_t *vis_in, const int32_t *source,
                const int32_t *auto_source, const uint8_t *channel_flags, void *vis,
                uint8_t *input_flags, float *weights, int channels, int in_baselines,
                int baselines, int vis_in_stride, int vis_stride, int input_flags_stride,
                int weights_stride, float scale, float weight_scale, int lost_flag);

/* prepare with flags per baseline: ksp_prepare and two more sources of input_flags, in the
 * same launch (bit for bit what rfi/host.py PrepareHost computes with mask_index and
 * baseline_flags). Everything said of ksp_prepare holds; in addition, for channel c and output
 * baseline j:
 *   cf = mask_classes == 0 ? (channel_flags ? channel_flags[c] : 0)
 *      : mask_index[j] < mask_classes ? channel_flags[mask_index[j]][c] : 0;
 *   input_flags = cf | (baseline_flags ? baseline_flags[j] : 0) | (lost ? lost_flag : 0).
 * mask_classes is 0 .. 8. With 0, mask_index is NULL, channel_flags (may be NULL) is one row
 * of uint8 [channels] and channel_flags_stride is ignored: with baseline_flags NULL as well
 * this is ksp_prepare. With 1 .. 8, channel_flags is uint8 [mask_classes][channel_flags_stride]
 * (a stride of at least channels, in elements) and must be given, as must mask_index, uint8
 * [baselines]: the class of static mask of every output baseline. Any uint8 is allowed in it:
 * a value of mask_classes or more (255, say) means "no static mask for this baseline" and is
 * never used to form an address. baseline_flags (uint8 [baselines], may be NULL) is ORed
 * into every sample of its baseline; vis and weights do not depend on it. Elements between
 * channels and channel_flags_stride are never read. The 16-byte paths need mask_index and
 * baseline_flags, where given, to be multiples of 16 bytes as well. Every argument is checked
 * before any device call. */
int ksp_prepare_flags(int device, void *stream, const int32_t *vis_in, const int32_t *source,
                      const int32_t *auto_source, const uint8_t *channel_flags,
                      const uint8_t *mask_index, const uint8_t *baseline_flags, void *vis,
                      uint8_t *input_flags, float *weights, int channels, int in_baselines,
                      int baselines, int mask_classes, int vis_in_stride,
                      int channel_flags_stride, int vis_stride, int input_flags_stride,
                      int weights_stride, float scale, float weight_scale, int lost_flag);

/* compress_weights: float32 weights as one byte per sample and one float32 per channel, in
 * one launch (no reference counterpart; bit for bit what rfi/host.py CompressWeightsHost
 * computes; every float step is one float32 operation, rounded once).
 * weights: float32 [channels][weights_stride]; weights8: uint8 [channels][weights8_stride];
 * baselines contiguous, strides in elements; weights_channel: float32 [channels].
 * Per channel c, with ok(w) = w > 0 and w < +inf:
 *   m  = max over b of (ok(weights[c][b]) ? weights[c][b] : +0);
 *   weights_channel[c] = wc = m / 255 (correctly rounded);
 *   t = weights[c][b] / wc (correctly rounded; IEEE when wc == 0);
 *   weights8[c][b] = !(weights[c][b] > 0) ? 0 : t >= 255 ? 255 : max(1, rint(t)), ties to even.
 * A byte is 0 exactly where the weight is zero, negative or NaN; +inf takes no part in the
 * maximum and becomes 255; with wc == 0 every positive weight becomes 255. Elements between
 * baselines and weights_stride are never read, elements between baselines and weights8_stride
 * never written. Rows of up to 32768 baselines are read once, longer rows twice. 16-byte loads
 * need weights and every row start of it to be multiples of 16 bytes, 16-byte stores the same
 * of weights8; anything else takes a slower element-wise path with the same result. No
 * workspace. Every argument is checked before any device call. */
int ksp_compress_weights(int device, void *stream, const float *weights, uint8_t *weights8,
                         float *weights_channel, int channels, int baselines,
                         int weights_stride, int weights8_stride);

/* apply_gains: per-input gain corrections applied to visibilities, weights and flags, in one
 * launch (no reference counterpart; bit for bit what rfi/host.py ApplyGainsHost computes;
 * every float step is one float32 operation, rounded once, a multiply then an add, never an
 * fma).
 * vis, out_vis: complex64 [channels][stride]; weights, out_weights: float32; flags, out_flags:
 * uint8; gains: complex64 [channels][gains_stride], of which n_inputs per row are data: the
 * correction that multiplies; inputs: int32 [baselines][2], contiguous: the two inputs of every
 * baseline. Baselines contiguous, one stride per array, in elements. Per channel c and
 * baseline j, with a = inputs[j][0], b = inputs[j][1]:
 *   inr = 0 <= a < n_inputs and 0 <= b < n_inputs;  ga = gains[c][a], gb = gains[c][b];
 *   cr = ga.re gb.re + ga.im gb.im;  ci = ga.im gb.re - ga.re gb.im;        (ga conj(gb))
 *   ok = inr and neither cr nor ci is NaN;  p = cr cr + ci ci;
 *   out_vis[c][j] = ok ? (v.re cr - v.im ci, v.re ci + v.im cr) : v, v = vis[c][j];
 *   out_weights[c][j] = ok and p > 0 ? weights[c][j] / p : 0 (correctly rounded);
 *   out_flags[c][j] = flags[c][j] | (ok ? 0 : flag_value).
 * Any int32 is allowed in inputs: an index outside 0 .. n_inputs - 1 is never used to form an
 * address, and its samples are treated like those of a NaN gain: vis passes through bit for
 * bit, the weight becomes 0 and flag_value is set. weights and out_weights are both NULL or
 * both given, and so are flags and out_flags. An output may be its input (the same pointer
 * with the same stride: in place); otherwise it must share no byte with it. gains and inputs
 * must not overlap any output. n_inputs is 1..4096, flag_value 1..255, channels and baselines
 * at least 1. Elements between baselines (or n_inputs) and a stride are neither read nor
 * written. 16-byte accesses need every sample array given, and every row start of it, to be a
 * multiple of 16 bytes (and inputs to be one, for its own loads); anything else takes a slower
 * element-wise path with the same result. One kernel launch, no workspace. Every argument is
 * checked before any device call. */
int ksp_apply_gains(int device, void *stream, const void *vis, const float *weights,
                    const uint8_t *flags, const void *gains, const int32_t *inputs,
                    void *out_vis, float *out_weights, uint8_t *out_flags, int channels,
                    int baselines, int n_inputs, int vis_stride, int weights_stride,
                    int flags_stride, int gains_stride, int out_vis_stride,
                    int out_weights_stride, int out_flags_stride, int flag_value);

/* solve_gains: per-input complex gains solved per channel from averaged visibilities of a point
 * source at the phase centre, with StEFCal, in one launch (no reference counterpart; bit for bit
 * what rfi/host.py SolveGainsHost computes, whose docstring states every step; every float step
 * is one float32 operation, rounded once, a multiply then an add, never an fma; sums run in
 * blocks of 32 indices, ascending from +0, the block sums added in ascending order).
 * vis: complex64 [channels][vis_stride]; weights: float32, flags: uint8, same layout, each NULL
 * or given (w = 1 without weights); pairs: int32 [n_inputs][pairs_stride], of which only the
 * entries [p][q] with p < q are read: t > 0 is baseline t - 1 listed as (p, q), t < 0 is
 * baseline -t - 1 listed as (q, p), whose sample is conjugated, and 0 or |t| > baselines (any
 * int32, INT32_MIN included) is no baseline and forms no address; initial: complex64
 * [channels][initial_stride] or NULL (1 + 0j); gains: complex64 [channels][gains_stride];
 * iterations: int32 [channels]; status: uint8 [channels]. Strides in elements.
 * A sample is kept when its entry is valid, neither part of v is NaN, w > 0 and
 * (flags & mask) == 0. Per channel, k = 1 .. max_iterations:
 *   new[p] = sum_q A[p][q] g[q] / sum_q W[p][q] |g[q]|^2  (g[p] where the divisor is not > 0);
 *   k odd: g = new;  k even: g = (new + g) / 2, and the channel stops, converged, when
 *   sum_p |g[p] - old[p]|^2 <= tol2 * sum_p |g[p]|^2 over the inputs that have data.
 * Then, if reference >= 0, that input has data and its gain's magnitude m is positive and
 * finite, every gain is multiplied by conj(g[reference]) / m and the reference's imaginary part
 * becomes +0; with corrections != 0 the output is conj(g) / |g|^2 (NaN where |g|^2 is not > 0):
 * what ksp_apply_gains multiplies by; an input without data gets NaN + NaN j.
 * iterations[c] is the number of iterations run; status[c] has bit 0 for "not converged",
 * bit 1 for "no input has data", bit 2 for "not referenced" (reference == -1 included).
 * tol2 is the square of the relative tolerance, at least 0. n_inputs is 1..128, max_iterations
 * 1..1000, reference -1..n_inputs-1, mask 0..255, corrections 0 or 1, channels and baselines
 * at least 1. gains may be initial (the same pointer with the same stride); otherwise it must
 * share no byte with it. Elements between baselines (or n_inputs) and a stride are neither
 * read nor written. One workgroup per channel with the channel's matrix in LDS; one kernel
 * launch, no workspace, no atomics. Every argument is checked before any device call. */
int ksp_solve_gains(int device, void *stream, const void *vis, const float *weights,
                    const uint8_t *flags, const int32_t *pairs, const void *initial, void *gains,
                    int32_t *iterations, uint8_t *status, int channels, int baselines,
                    int n_inputs, int vis_stride, int weights_stride, int flags_stride,
                    int pairs_stride, int initial_stride, int gains_stride, int max_iterations,
                    float tol2, int reference, int mask, int corrections);

/* solve_gains_large: ksp_solve_gains for n_inputs 1..512 (bit for bit what rfi/host.py
 * SolveGainsLargeHost computes: the arithmetic of SolveGainsHost, with up to 16 block sums per
 * row and in the convergence sums; up to 128 inputs the results are those of ksp_solve_gains).
 * Every array, stride and setting is as for ksp_solve_gains, with the same rules for an entry
 * of pairs, the same kept-sample rule and the same status bits.
 * Above 128 inputs a channel's matrix (12 n_inputs^2 bytes) does not fit LDS and lives in
 * work_area, device memory the caller supplies: ksp_solve_gains_large_work_bytes(channels,
 * n_inputs) bytes, 4-byte aligned, sharing no byte with any other argument (all work_bytes of
 * it count). A fixed grid of G = min(256, channels) workgroups is launched, workgroup i solving
 * channels i, i + G, ... one after another in slot i of the work area, so
 *   work bytes = min(256, channels) * 12 * n_inputs * ld,  ld = n_inputs rounded up to 32,
 * at most 768 MiB (512 inputs, 256 or more channels). A slot is rewritten for every channel
 * before it is read: the work area need not be cleared, its contents after the call mean
 * nothing, nothing behind the needed bytes is touched, and it may be shared with anything that
 * does not run at the same time. The function gives 0 for channels < 1 and for n_inputs outside
 * 129..512: up to 128 inputs the call is handed to ksp_solve_gains after the checks, and
 * work_area and work_bytes are not looked at. One kernel launch, no atomics, no workgroup waits
 * for another. Every argument is checked before any device call. */
size_t ksp_solve_gains_large_work_bytes(int channels, int n_inputs);
int ksp_solve_gains_large(int device, void *stream, const void *vis, const float *weights,
                          const uint8_t *flags, const int32_t *pairs, const void *initial,
                          void *gains, int32_t *iterations, uint8_t *status, void *work_area,
                          size_t work_bytes, int channels, int baselines, int n_inputs,
                          int vis_stride, int weights_stride, int flags_stride, int pairs_stride,
                          int initial_stride, int gains_stride, int max_iterations, float tol2,
                          int reference, int mask, int corrections);

/* solve_jones: per-antenna 2x2 Jones matrices solved per channel from averaged visibilities of
 * an unpolarised unit source at the phase centre, with the full-polarisation StEFCal step, in
 * one launch (no reference counterpart; bit for bit what rfi/host.py SolveJonesHost computes,
 * whose docstring states every step and the order of the operations inside it; the rules for
 * float steps and for sums are those of ksp_solve_gains).
 * n_inputs is even; input 2a + i is feed i of antenna a. vis, weights, flags, pairs,
 * iterations and status are as for ksp_solve_gains, with the same kept-sample rule and the same
 * rules for an entry of pairs, and one more: an entry [p][q] with p / 2 == q / 2 (one antenna)
 * is no baseline. initial: complex64 [channels][initial_stride][2] or NULL (every matrix the
 * identity); jones: complex64 [channels][jones_stride][2]; row p = 2a + i holds
 * z_p = (J_a[i][0], J_a[i][1]), and the model is V[p][q] = z_p[0] conj(z_q[0]) +
 * z_p[1] conj(z_q[1]). initial_stride and jones_stride count rows of two complex64 (16
 * bytes); the other strides count elements. Per channel, k = 1 .. max_iterations:
 *   num[p] = sum_q A[p][q] z_q;  H[p] = sum_q W[p][q] z_q^H z_q (2x2, Hermitian);
 *   new[p] = num[p] H[p]^-1 where det H[p] > 0, else z_p;
 *   k odd: z = new;  k even: z = (new + z) / 2, and the channel stops, converged, when
 *   sum_p |z_p - old_p|^2 <= tol2 * sum_p |z_p|^2 over the inputs that have data.
 * Then, if reference >= 0 (an antenna), both of its inputs have data and the modulus of its
 * matrix's determinant is positive and finite, every row is multiplied by U^H, U the unitary
 * factor of that matrix's polar decomposition, which makes the reference's matrix Hermitian and
 * positive, and the imaginary parts of its diagonal become +0 (for an unpolarised source this
 * choice of U is a convention that the data cannot check); with corrections != 0 every
 * antenna's matrix is replaced by its inverse adj(J) / det J (NaN where |det J|^2 is not > 0 or
 * either input has no data); without corrections the rows of inputs without data are
 * NaN + NaN j. status[c] has bit 0 for "not converged", bit 1 for "no input has data", bit 2
 * for "not referenced" (reference == -1 included) and bit 3 for "in the last iteration an input
 * with data kept its row because det H was not above 0".
 * n_inputs is even and 2..128, max_iterations 1..1000, tol2 at least 0, reference
 * -1..n_inputs/2-1, mask 0..255, corrections 0 or 1, channels and baselines at least 1. jones
 * may be initial (the same pointer with the same stride); otherwise it must share no byte with
 * it; both need the alignment of a complex64 only. Elements between baselines (or n_inputs)
 * and a stride are neither read nor written. One workgroup per channel with the channel's
 * matrix in LDS; one kernel launch, no workspace, no atomics. Every argument is checked before
 * any device call. */
int ksp_solve_jones(int device, void *stream, const void *vis, const float *weights,
                    const uint8_t *flags, const int32_t *pairs, const void *initial, void *jones,
                    int32_t *iterations, uint8_t *status, int channels, int baselines,
                    int n_inputs, int vis_stride, int weights_stride, int flags_stride,
                    int pairs_stride, int initial_stride, int jones_stride, int max_iterations,
                    float tol2, int reference, int mask, int corrections);

/* apply_jones: per-antenna 2x2 Jones corrections applied to visibilities, weights and flags,
 * C_a V_ab C_b^H on the four products of every antenna pair, in one launch (no reference
 * counterpart; bit for bit what rfi/host.py ApplyJonesHost computes, whose docstring states
 * every step and the order of the operations inside it; every float step is one float32
 * operation, rounded once, a multiply then an add, never an fma; correctly rounded division).
 * vis, out_vis: complex64 [channels][stride]; weights, out_weights: float32; flags, out_flags:
 * uint8; jones: complex64 [channels][jones_stride][2] as ksp_solve_jones writes it (with
 * corrections != 0, the matrices that multiply), of which n_inputs rows per channel are data:
 * row 2a + i is row i of antenna a's matrix C_a. jones_stride counts rows of two complex64 (16
 * bytes); the other strides count elements. quad_antennas: int32 [n_quads][2], contiguous: the
 * antennas (a, b) of every quad; quads: int32 [n_quads][4], contiguous: its entries (t00, t01,
 * t10, t11), where t at (m, n) follows the rules of ksp_solve_gains' pairs: t > 0 is baseline
 * t - 1 listed as (2a+m, 2b+n), t < 0 is baseline -t - 1 listed the other way round, whose
 * imaginary part is negated on load and again on store, and 0 or |t| > baselines (any int32,
 * INT32_MIN included) is absent and forms no address. With a == b an absent (1,0) beside a
 * present (0,1) reads as the conjugate of that sample, with its weight and flags, and the
 * other way round. Per channel c and quad:
 *   complete = 0 <= a, b < n_inputs / 2 and all four sources are there (a stand-in counts);
 *   ok = complete and none of the 16 floats of rows 2a, 2a+1, 2b, 2b+1 of jones[c] is NaN;
 *   T[i][n] = C_a[i][0] S[0][n] + C_a[i][1] S[1][n];
 *   O[i][k] = T[i][0] conj(C_b[k][0]) + T[i][1] conj(C_b[k][1]);
 *   u[i][n] = |C_a[i][0]|^2 / w[0][n] + |C_a[i][1]|^2 / w[1][n]   (1 / w first, then the product);
 *   var[i][k] = u[i][0] |C_b[k][0]|^2 + u[i][1] |C_b[k][1]|^2;
 *   for every entry (i, k) that is present itself, at its baseline j:
 *   out_vis[c][j] = ok ? O[i][k] : vis[c][j];
 *   out_weights[c][j] = ok and every w > 0 and var[i][k] > 0 ? 1 / var[i][k] : 0;
 *   out_flags[c][j] = OR of the flags of the present sources | (ok ? 0 : flag_value).
 * A baseline that no present entry names is neither read nor written. A baseline named by two
 * present entries is the caller's breach: those baselines are undefined, nothing else is. An
 * antenna outside 0 .. n_inputs / 2 - 1 (any int32) forms no address: its quad is not complete.
 * weights and out_weights are both NULL or both given, and so are flags and out_flags. An
 * output may be its input (the same pointer with the same stride: in place); otherwise it must
 * share no byte with it. jones and the two tables must not overlap any output; jones needs the
 * alignment of a complex64 only. n_inputs is even and 2..2048, n_quads, channels and baselines
 * at least 1, flag_value 1..255. Elements between baselines (or n_inputs) and a stride are
 * neither read nor written. One kernel launch, no workspace, no atomics. Every argument is
 * checked before any device call. */
int ksp_apply_jones(int device, void *stream, const void *vis, const float *weights,
                    const uint8_t *flags, const void *jones, const int32_t *quad_antennas,
                    const int32_t *quads, void *out_vis, float *out_weights, uint8_t *out_flags,
                    int channels, int baselines, int n_inputs, int n_quads, int vis_stride,
                    int weights_stride, int flags_stride, int jones_stride, int out_vis_stride,
                    int out_weights_stride, int out_flags_stride, int flag_value);

/* predict: model visibilities of up to 64 point sources and, optionally, the data divided by
 * them, in one launch: the step in front of ksp_solve_gains for a calibrator that is not a unit
 * source at the phase centre (no reference counterpart; bit for bit what rfi/host.py
 * PredictHost computes; every step is one operation, rounded once, a multiply then an add,
 * never an fma: float64 for the model, float32 for the division).
 * freqs: float64 [channels], Hz; delays: float64 [n_sources][delays_stride], seconds, of which
 * baselines per row are data; flux: float32 [channels][flux_stride], of which n_sources per row
 * are data; model, vis, out_vis: complex64 [channels][stride]; weights, out_weights: float32;
 * flags, out_flags: uint8. Baselines contiguous, one stride per array, in elements. Per
 * channel c, baseline j and source s, in float64:
 *   x = freqs[c] delays[s][j];  r = x - rint(x);  q = rint(4 r);  y = r - q 0.25;
 *   z = y 6.283185307179586;  z2 = z z;
 *   sn = (((((S5 z2 + S4) z2 + S3) z2 + S2) z2 + S1) z2 + S0) z;
 *   cs = (((((C6 z2 + C5) z2 + C4) z2 + C3) z2 + C2) z2 + C1) z2 + C0;
 *     S0..S5 = 1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984,
 *              2.7557319223985893e-06, -2.505210838544172e-08;
 *     C0..C6 = 1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05,
 *              -2.755731922398589e-07, 2.08767569878681e-09;
 *   (co, si) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs) for q = 0, 1, +-2, -1;
 *   re += flux[c][s] co;  im -= flux[c][s] si     (from +0, s ascending);
 * model[c][j] = M = (float32(re), float32(im)), to nearest. With vis, in float32:
 *   d = M.re M.re + M.im M.im;  ok = 0 < d < inf;
 *   out_vis[c][j] = ok ? ((v.re M.re + v.im M.im) / d, (v.im M.re - v.re M.im) / d) : v;
 *   out_weights[c][j] = ok ? weights[c][j] d : 0;
 *   out_flags[c][j] = flags[c][j] | (ok ? 0 : flag_value).
 * NaN and infinities go through as IEEE gives them: a non-finite x gives a NaN model, and a
 * sample whose model is zero, NaN, or has a d that underflows or overflows keeps its vis bit
 * for bit, gets weight 0 and flag_value. model may be NULL if vis is given, and vis if model
 * is; out_vis is given exactly when vis is; weights and out_weights are both NULL or both
 * given, and only with vis; so are flags and out_flags. An output may be its input (the same
 * pointer with the same stride: in place); otherwise it must share no byte with it. model
 * must share no byte with any other array. n_sources is 1..64, flag_value 1..255, channels and
 * baselines at least 1. Elements between baselines (or n_sources) and a stride are neither
 * read nor written. 16-byte accesses need every sample array given (model included), and
 * every row start of it, to be a multiple of 16 bytes; anything else takes a slower
 * element-wise path with the same result. One kernel launch, no workspace, no atomics. Every
 * argument is checked before any device call. */
int ksp_predict(int device, void *stream, const double *freqs, const double *delays,
                const float *flux, void *model, const void *vis, const float *weights,
                const uint8_t *flags, void *out_vis, float *out_weights, uint8_t *out_flags,
                int channels, int baselines, int n_sources, int delays_stride, int flux_stride,
                int model_stride, int vis_stride, int weights_stride, int flags_stride,
                int out_vis_stride, int out_weights_stride, int out_flags_stride,
                int flag_value);

/* fit_delays: per input, the delay and phase whose phasor best matches the gains that
 * ksp_solve_gains leaves across the band, and that phasor for every channel of the band, which
 * is what ksp_apply_gains applies, in one launch (no reference counterpart; bit for bit what
 * rfi/host.py FitDelaysHost computes; every step is one operation, rounded once, a multiply
 * then an add, never an fma: float32 for the transform, float64 for the refinement).
 * gains, model: complex64 [channels][stride], of which n_inputs per row are data; status:
 * uint8 [channels] or NULL; delays: float64 [n_inputs], seconds; phasors: complex64
 * [n_inputs]; amplitudes: float32 [n_inputs]; fit_status: uint8 [n_inputs]. Per input p:
 *   x[c] = gains[c][p] if both parts are finite and (status is NULL or
 *   status[c] & status_mask == 0), else 0; x[c] = 0 for c = channels .. n_fft - 1; n_kept
 *   counts the kept channels.
 *   Coarse, float32: X = the in-place radix-2 decimation-in-time transform of x with
 *   W = exp(-2 pi i / n_fft): bit reversal, then stages s = 1 .. log2 n_fft, half = 2^(s-1),
 *   butterfly (j, j + half) with tw = (float32(co), float32(-si)), (co, si) the cos_sin of
 *   ksp_predict at (j mod half) / 2^s turns:
 *     bt = (b.re tw.re - b.im tw.im, b.re tw.im + b.im tw.re);  a' = a + bt;  b' = a - bt;
 *   P[k] = re re + im im; k0 = the lowest k at which P takes its largest value that is not NaN.
 *   No fit (bit 0 of fit_status) if n_kept < 2, every P is NaN or that value is not in (0, inf).
 *   Refinement, float64, from nu = k0 / n_fft, `refine` times: per kept channel
 *     (co, si) = cos_sin(c nu);  e = (x.re co + x.im si, x.im co - x.re si);
 *     D0 = sum e;  D1 = sum c e;  D2 = sum (c c) e, each the halving tree over Cpad terms
 *     (the next power of two at or above channels; other terms +0):
 *     n = Cpad; while n > 1: n /= 2, t[i] = t[i] + t[i + n] for i < n;
 *     num = D1.im D0.re - D1.re D0.im;
 *     den = 6.283185307179586 ((D1.re D1.re + D1.im D1.im) - (D2.re D0.re + D2.im D0.im));
 *     step = num / den;  if den < 0 and |step| <= 1 / n_fft then nu = nu - step, else bit 1 of
 *     fit_status is set and the loop ends (a NaN fails both tests).
 *   Results, from D0 at the final nu: m = sqrt(D0.re D0.re + D0.im D0.im); no fit unless m is
 *   in (0, inf); phasors[p] = (float32(D0.re / m), float32(D0.im / m));
 *   amplitudes[p] = float32(m / n_kept); delays[p] = (nu - rint(nu)) / channel_width; and
 *   with ph the rounded phasor and (co, si) = cos_sin(c nu), for every c < channels,
 *   model[c][p] = (float32(ph.re co - ph.im si), float32(ph.re si + ph.im co)), the imaginary
 *   part negated if corrections is 1. An input without a fit has NaN in delays, phasors,
 *   amplitudes and its column of model.
 * status and model may be NULL. channels is 1..8192, n_inputs at least 1, n_fft a power of two
 * in 4..16384 and at least twice the channels, refine 0..8, status_mask 0..255, corrections 0
 * or 1, channel_width finite and not 0. model must share no byte with gains. Elements between
 * n_inputs and a stride are neither read nor written. One kernel launch, one workgroup per
 * input with 8 n_fft bytes of LDS, no workspace, no atomics. Every argument is checked before
 * any device call. */
int ksp_fit_delays(int device, void *stream, const void *gains, const uint8_t *status,
                   double *delays, void *phasors, float *amplitudes, uint8_t *fit_status,
                   void *model, int channels, int n_inputs, int gains_stride, int model_stride,
                   int n_fft, int refine, int status_mask, int corrections,
                   double channel_width);

/* interpolate_gains: per input, the gains that ksp_solve_gains leaves, filled across the
 * channels it left without a value, as a table that ksp_apply_gains can apply to another scan,
 * in one launch (no reference counterpart; bit for bit what rfi/host.py InterpolateGainsHost
 * computes; every step is one float32 operation, rounded once, a multiply then an add, never an
 * fma, real and imaginary parts apart, division and square root correctly rounded; a complex
 * product a b is (a.re b.re - a.im b.im, a.re b.im + a.im b.re)).
 * gains, model, out: complex64 [channels][stride], of which n_inputs per row are data; status:
 * uint8 [channels] or NULL; model: what ksp_fit_delays writes with corrections 0 (taken as unit
 * modulus), or NULL; scale: complex64 [n_inputs] or NULL; kept, filled: int32 [n_inputs];
 * fill_status: uint8 [n_inputs]; mean_amplitude: float32 [n_inputs], or NULL for no
 * normalisation. Per input p, with g = gains[c][p] and m = model[c][p]:
 *   1. c is kept if both parts of g are finite, (status is NULL or status[c] & status_mask == 0)
 *      and (model is NULL or both parts of m are finite), else missing; kept[p] counts the kept
 *      ones; none: bit 0 of fill_status[p].
 *   2. d = (g.re m.re + g.im m.im, g.im m.re - g.re m.im), or g without model.
 *   3. for a kept c, s[c] = the sum of d over the kept channels of [c - smooth / 2,
 *      c + smooth / 2] inside the band, added in ascending order from +0, divided by float of
 *      their number; smooth == 1: s = d, no sum and no division.
 *   4. with mean_amplitude: a = (the sum of sqrt(s.re s.re + s.im s.im) over the kept channels
 *      as the halving tree over Cpad terms, the next power of two at or above channels, other
 *      terms +0: n = Cpad; while n > 1: n /= 2, t[i] = t[i] + t[i + n] for i < n)
 *      / float(kept[p]); mean_amplitude[p] = a, NaN if no channel is kept; a in (0, inf):
 *      s = (s.re / a, s.im / a), else bit 0.
 *   5. y[c] = s[c] for a kept c. For a missing c, with l the nearest kept channel below and r
 *      the nearest above: both and r - l - 1 <= max_gap: t = float(c - l) / float(r - l),
 *      y = s[l] + (s[r] - s[l]) t per part; only l and c - l <= max_gap: y = s[l]; only r and
 *      r - c <= max_gap: y = s[r]; otherwise y = NaN and bit 1 of fill_status[p]. filled[p]
 *      counts the missing channels that got a value.
 *   6. with model, y = y m at every channel;  7. with scale, y = y scale[p];
 *   8. corrections 1: q = y.re y.re + y.im y.im, out = q > 0 ? (y.re / q, -y.im / q) : NaN.
 *   An input with bit 0 has NaN in its column of out, filled[p] = 0 and no other bit.
 * channels is 1..16384, n_inputs at least 1, max_gap 0..16384, smooth odd and 1..31,
 * status_mask 0..255, corrections 0 or 1. out may be gains itself (same pointer and stride) but
 * must not overlap it otherwise, and shares no byte with model. Elements between n_inputs and a
 * stride are neither read nor written. One kernel launch, one workgroup per input with
 * 8 channels bytes of LDS, no workspace, no atomics. Every argument is checked before any
 * device call. */
int ksp_interpolate_gains(int device, void *stream, const void *gains, const uint8_t *status,
                          const void *model, const void *scale, void *out, int *kept,
                          int *filled, uint8_t *fill_status, float *mean_amplitude,
                          int channels, int n_inputs, int gains_stride, int model_stride,
                          int out_stride, int max_gap, int smooth, int status_mask,
                          int corrections);

/* interpolate_jones: per antenna, the 2x2 matrices that ksp_solve_jones leaves (corrections 0),
 * filled across the channels it left without a matrix, as a table that ksp_apply_jones can
 * apply to another scan, in one launch: the 2x2 counterpart of ksp_interpolate_gains, with its
 * arithmetic (no reference counterpart; bit for bit what rfi/host.py InterpolateJonesHost
 * computes; every step one float32 operation, rounded once, never an fma).
 * jones, out: complex64 [channels][stride][2], of which n_inputs rows of two per channel are
 * data: row 2a + i is row i of antenna a's matrix, and the strides count such rows, as in
 * ksp_solve_jones; model: complex64 [channels][model_stride], what ksp_fit_delays writes with
 * corrections 0, or NULL; status: uint8 [channels] or NULL; scale: complex64 [n_inputs] or
 * NULL; kept, filled: int32 [n_inputs / 2]; fill_status: uint8 [n_inputs / 2]; mean_amplitude:
 * float32 [n_inputs / 2], or NULL for no normalisation. Per antenna a, with
 * z[i][k] = jones[c][2a + i][k] and m_i = model[c][2a + i]:
 *   1. c is kept if all eight floats of z are finite, (status is NULL or
 *      status[c] & status_mask == 0) and (model is NULL or all four floats of m_0 and m_1 are
 *      finite), else missing: one mask per antenna; kept[a] counts the kept ones; none: bit 0
 *      of fill_status[a].
 *   2. d[i][k] = z[i][k] conj(m_i) as step 2 of ksp_interpolate_gains, or z without model.
 *   3. per element, step 3 of ksp_interpolate_gains (the four elements share the count).
 *   4. with mean_amplitude: nik = s[i][k].re s[i][k].re + s[i][k].im s[i][k].im;
 *      term = sqrt(((n00 + n01) + (n10 + n11)) 0.5) per kept channel; a = (the halving tree of
 *      ksp_interpolate_gains over Cpad terms) / float(kept[a]); mean_amplitude[a] = a, NaN if
 *      no channel is kept; a in (0, inf): all eight floats of s are divided by a, else bit 0.
 *   5. per element, step 5 of ksp_interpolate_gains with one l, r and t for the four elements;
 *      filled[a] counts the missing channels that got a matrix; a gap left is bit 1.
 *   6. with model, y[i][k] = y[i][k] m_i at every channel;
 *   7. with scale, y[i][k] = y[i][k] scale[2a + i];
 *   8. corrections 1: D = y00 y11 - y01 y10; q = D.re D.re + D.im D.im;
 *      inv = (D.re / q, -D.im / q); out = [[y11 inv, -(y01 inv)], [-(y10 inv), y00 inv]] (the
 *      products are negated), NaN in all four elements unless q > 0.
 *   An antenna with bit 0 has NaN in all its elements of out, filled[a] = 0 and no other bit.
 * channels is 1..16384, n_inputs even and 2..2048, max_gap 0..16384, smooth odd and 1..31,
 * status_mask 0..255, corrections 0 or 1. out may be jones itself (same pointer and stride) but
 * must not overlap it otherwise, and shares no byte with model. jones and out need the
 * alignment of a complex64 only. Rows between n_inputs and a stride are neither read nor
 * written. One kernel launch, one workgroup per antenna with 8 channels bytes of LDS, no
 * workspace, no atomics. Every argument is checked before any device call. */
int ksp_interpolate_jones(int device, void *stream, const void *jones, const uint8_t *status,
                          const void *model, const void *scale, void *out, int *kept,
                          int *filled, uint8_t *fill_status, float *mean_amplitude,
                          int channels, int n_inputs, int jones_stride, int model_stride,
                          int out_stride, int max_gap, int smooth, int status_mask,
                          int corrections);

/* jones_diagonal: gains[c][p] = jones[c][p][p % 2], a copy of bits: the diagonal of every
 * antenna's matrix as the per-input gains that ksp_fit_delays reads. jones: complex64
 * [channels][jones_stride][2] (strides in rows of two, as above); gains: complex64
 * [channels][gains_stride]. channels and n_inputs are at least 1; gains shares no byte with
 * jones. Elements between n_inputs and a stride are neither read nor written. One kernel
 * launch. Every argument is checked before any device call. */
int ksp_jones_diagonal(int device, void *stream, const void *jones, void *gains, int channels,
                       int n_inputs, int jones_stride, int gains_stride);

/* range_percentiles: per channel and per range of baselines, the [0, 100, 25, 75, 50] %
 * amplitudes ("lower" element) of the samples that are neither NaN nor flagged under a mask,
 * how many those are, and the OR of the range's flags, all ranges in one launch (no reference
 * counterpart; bit for bit what rfi/host.py RangePercentilesHost computes; with nothing left
 * out, what ksp_percentile5_float gives for the same column range).
 * in: [channels][in_stride] float32 amplitudes (is_amplitude != 0) or complex64 (== 0), of
 * which `baselines` are data; flags: uint8 [channels][flags_stride]. percentiles: float32
 * [n_ranges * 5][out_stride], counts: uint32 [n_ranges][counts_stride], range_flags: uint8
 * [n_ranges][range_flags_stride], of which `channels` per row are data. Strides in elements.
 * ranges is a HOST pointer to n_ranges (1..16) pairs (start, stop) of ints with
 * 0 <= start <= stop <= baselines and stop - start <= 16384; it is copied during the call.
 * Ranges may be empty, overlap, repeat and come in any order. Per channel c and range r:
 *   a[b] = in[c][b], or numpy's |in[c][b]| for complex64              (b in [start, stop));
 *   kept = { b : a[b] is not NaN and (flags[c][b] & mask) == 0 },  n = size of kept;
 *   counts[r][c] = n;  with K the kept a[b] in ascending order,
 *   percentiles[5 r + 0 .. 5 r + 4][c] = K[0], K[n-1], K[(n-1)/4], K[3(n-1)/4], K[(n-1)/2],
 *   five +0.0 when n == 0;  range_flags[r][c] = OR of flags[c][b] over ALL b of the range.
 * flags and range_flags are both NULL (then mask must be 0 and flags_stride and
 * range_flags_stride are ignored) or both given; mask is 0..255. float32 input must be
 * non-negative with the sign bit clear, or NaN (+inf is an ordinary largest value); anything
 * else gives an unspecified value in that range's percentiles and no access outside the
 * arrays. Every output element inside [row * stride, row * stride + channels) is written on
 * every call; elements beyond `channels` of an output row are never written, elements outside
 * the ranges of an input row never read. 16-byte loads are taken where the first sample and
 * first flag byte of a range in a row allow it; anything else goes element by element with
 * the same result. One kernel launch, no workspace. channels == 0 returns 0. Every argument
 * is checked before any device call. */
int ksp_range_percentiles(int device, void *stream, const void *in, const unsigned char *flags,
                          float *percentiles, unsigned *counts, unsigned char *range_flags,
                          int channels, int baselines, int in_stride, int flags_stride,
                          int out_stride, int counts_stride, int range_flags_stride,
                          const int *ranges, int n_ranges, int is_amplitude, int mask);

/* band_average: per baseline and per series of channel weights (1..8 series), the weighted
 * mean of the visibility and of its amplitude over the channels whose samples are neither NaN
 * nor flagged under a mask, the weight sum, the number of samples kept and the OR of the flags
 * of the series' channels; every sample is read once for all series (no reference
 * counterpart; bit for bit what rfi/host.py BandAverageHost computes).
 * data: complex64 [channels][data_stride], flags: uint8 [channels][flags_stride], of which
 * `baselines` per row are data; channel_weights: float32 [n_series][channel_weights_stride],
 * of which `channels` per row are data. mean: complex64 [n_series][mean_stride];
 * mean_amplitude, weight_sums: float32, counts: uint32, series_flags: uint8, each
 * [n_series][its stride], of which `baselines` per row are data. Strides in elements.
 * For series k and baseline b, every step one float32 operation, rounded once (a multiply,
 * then an add: never an fma), with w = channel_weights[k][c]:
 *   in_k = w > 0 (a zero, negative or NaN weight leaves channel c out of series k);
 *   kept = in_k and neither part of data[c][b] is NaN and (flags[c][b] & mask) == 0;
 *   a = numpy's |data[c][b]|;
 *   per block j of 128 consecutive channels (the last may be short), from +0.0, over the kept
 *   c in ascending order: p_re += w * re, p_im += w * im, p_a += w * a, p_w += w;
 *   S_re, S_im, S_a, S_w = the block partials added in ascending j from +0.0;
 *   counts[k][b] = number of kept samples; series_flags[k][b] = OR of flags[c][b] over ALL c
 *   with in_k; weight_sums[k][b] = S_w; mean[k][b] = S_w > 0 ? (S_re / S_w, S_im / S_w) : 0;
 *   mean_amplitude[k][b] = S_w > 0 ? S_a / S_w : 0.
 * flags and series_flags are both NULL (then mask must be 0 and their strides are ignored) or
 * both given; mask is 0..255; channels is 1..262144, baselines at least 1. work_area is
 * device memory of at least ksp_band_average_work_bytes(channels, baselines, n_series) =
 * ceil(channels / 128) * n_series * 5 * baselines * 4 bytes (0 for sizes outside the limits),
 * 4-byte aligned; it need not be cleared and holds nothing of use after the call; work_bytes
 * is its size. Two kernel launches (block partials, then their ordered sum), no atomics.
 * A sample is one 8-byte load and a flag one byte, whatever the alignment of the rows beyond
 * that of their types. Elements beyond `baselines` of a row are never read or written. Every argument is checked
 * before any device call. */
size_t ksp_band_average_work_bytes(int channels, int baselines, int n_series);
int ksp_band_average(int device, void *stream, const void *data, const unsigned char *flags,
                     const float *channel_weights, void *mean, float *mean_amplitude,
                     float *weight_sums, unsigned *counts, unsigned char *series_flags,
                     void *work_area, size_t work_bytes, int channels, int baselines,
                     int n_series, int data_stride, int flags_stride,
                     int channel_weights_stride, int mean_stride, int mean_amplitude_stride,
                     int weight_sums_stride, int counts_stride, int series_flags_stride,
                     int mask);

/* ---- masked_gaussian_filter (reference rfi/twodflag.py:254-400) ----
 * Images [images][rows][cols] of float32 (itemsize 4) or float64 (itemsize 8); data, flags
 * (uint8, non-zero = flagged) and out share image_stride and row_stride, in elements
 * (columns contiguous). r0 / r1: box radius along axis 0 / axis 1 (0 = not filtered along
 * that axis); divisor0 / divisor1: (2 r + 1) ** passes as numba computes it, by squaring
 * and multiplying in the data's type (any positive value where the radius is 0).
 * out = NaN where the filtered weight is 0, else filtered masked data / filtered weight,
 * bit for bit the reference's result. out may be the same buffer as data.
 * Limits: rows, cols 1..65536; passes 1..8; radii 0..2047; with passes = 1 a radius may
 * not exceed the length of its axis. Every argument is checked before any device call.
 * ksp_masked_filter_workspace: bytes of device workspace for batches of `batch` images.
 * ksp_masked_filter: filters images [image0, image0 + batch). */
int ksp_masked_filter_workspace(int rows, int cols, int batch, int r0, int r1, int passes,
                                int itemsize, size_t *bytes);
int ksp_masked_filter(int device, void *stream, const void *data, const uint8_t *flags, void *out,
                      int rows, int cols, int images, long long image_stride,
                      long long row_stride, int image0, int batch, int r0, int r1, int passes,
                      double divisor0, double divisor1, int itemsize, void *workspace,
                      size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* KATSDPSIGPROC_HIP_H */
