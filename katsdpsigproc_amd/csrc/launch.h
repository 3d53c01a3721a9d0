// Host-side launch helpers: a run-time integer or bool as a template argument, the array
// arguments of a launcher as one list of planes (NULL, stride and the alignment test of the
// 16-byte load paths, each written once), the test of an output that may be its input, the
// grid of the kernels that deal runs to threads, what a launcher does once per device, and the
// choice between a plain and an event-timed launch. No device code.
#pragma once
#include <hip/hip_ext.h>

#include <atomic>
#include <initializer_list>
#include <type_traits>

#include "ksp_common.h"

// Returns the code of a helper that failed and has said why with ksp_set_error.
#define KSP_TRY(expr)              \
    do {                           \
        const int _rc = (expr);    \
        if (_rc != 0) return _rc;  \
    } while (0)

// A run-time integer as a template argument: f(std::integral_constant<int, V>()) for the V of
// Vs... that equals `value` (exact), or for the first V that `value` does not exceed (ceil:
// Vs... ascending). Returns whether there was such a V; f's own result is dropped.
template <int... Vs, typename F>
inline bool ksp_dispatch_exact(int value, F &&f)
{
    return ((value == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}
template <int... Vs, typename F>
inline bool ksp_dispatch_ceil(int value, F &&f)
{
    return ((value <= Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}
// The same for a bool: f(std::true_type()) or f(std::false_type()).
template <typename F>
inline void ksp_dispatch_bool(bool value, F &&f)
{
    if (value)
        f(std::true_type());
    else
        f(std::false_type());
}

// Whether rows that start at `ptr` and lie `stride` elements of `elem_bytes` bytes apart can
// be read in pieces of `bytes` bytes: every row starts on a multiple of `bytes`.
inline bool ksp_rows_aligned(const void *ptr, long long stride, int elem_bytes, int bytes = 16)
{
    return (uintptr_t)ptr % bytes == 0 && stride * elem_bytes % bytes == 0;
}

// One [rows][stride] array argument as a launcher's checks see it: its name in the header,
// the pointer (NULL: not given), the row stride in elements (0 for a one-dimensional array)
// and the bytes of an element. `optional` arrays may be left out by the caller. A launcher
// states each array once, in a list in the order of its checks, and hands the list (or part
// of it) to the three functions below.
struct ksp_plane {
    const char *name;
    const void *ptr;
    long long stride;
    int elem_bytes;
    bool optional = false;
};
using ksp_planes = std::initializer_list<ksp_plane>;

// "<name> is NULL" for the first plane that is not given and not optional.
inline int ksp_planes_given(ksp_planes planes)
{
    for (const ksp_plane &p : planes)
        if (p.ptr == nullptr && !p.optional) {
            ksp_set_error("invalid argument: %s is NULL", p.name);
            return (int)hipErrorInvalidValue;
        }
    return 0;
}

// "<name>_stride is smaller than <what>" for the first given plane whose rows are shorter
// than `cols` elements.
inline int ksp_planes_hold(ksp_planes planes, long long cols, const char *what)
{
    for (const ksp_plane &p : planes)
        if (p.ptr != nullptr && p.stride < cols) {
            ksp_set_error("invalid argument: %s_stride is smaller than %s", p.name, what);
            return (int)hipErrorInvalidValue;
        }
    return 0;
}

// Whether every given plane passes ksp_rows_aligned: the kernel may use 16-byte accesses.
inline bool ksp_planes_aligned(ksp_planes planes)
{
    for (const ksp_plane &p : planes)
        if (p.ptr != nullptr && !ksp_rows_aligned(p.ptr, p.stride, p.elem_bytes)) return false;
    return true;
}

// Whether two planes, each with its rows and the columns of a row that are data, share no byte.
inline bool ksp_planes_apart(const ksp_plane &a, long long a_rows, long long a_cols,
                             const ksp_plane &b, long long b_rows, long long b_cols)
{
    const uintptr_t a0 = (uintptr_t)a.ptr, b0 = (uintptr_t)b.ptr;
    const uintptr_t a1 = a0 + (uintptr_t)(((a_rows - 1) * a.stride + a_cols) * a.elem_bytes);
    const uintptr_t b1 = b0 + (uintptr_t)(((b_rows - 1) * b.stride + b_cols) * b.elem_bytes);
    return a1 <= b0 || b1 <= a0;
}

// The inputs of a kernel that an output each goes with, as a list {in, out, in, out, ...}: an
// optional input and its output are given together or not at all, and an output is its input
// (same pointer, same stride: in place) or shares no byte with it. The two checks are apart
// because a launcher has others between them.
// "<in> and <out> must both be NULL or both be given" for the first pair with one of the two.
inline int ksp_pairs_given_together(ksp_planes pairs)
{
    for (const ksp_plane *p = pairs.begin(); p != pairs.end(); p += 2)
        if ((p[0].ptr == nullptr) != (p[1].ptr == nullptr)) {
            ksp_set_error(
                "invalid argument: %s and %s must both be NULL or both be given "
                "((%s == nullptr) == (%s == nullptr))",
                p[0].name, p[1].name, p[0].name, p[1].name);
            return (int)hipErrorInvalidValue;
        }
    return 0;
}

// "<out> overlaps <in> without being <in> with the same stride" for the first given pair that
// is neither; `cols` elements of each of the `rows` rows are data.
inline int ksp_pairs_same_or_apart(ksp_planes pairs, long long rows, long long cols)
{
    for (const ksp_plane *p = pairs.begin(); p != pairs.end(); p += 2)
        if (p[0].ptr != nullptr && !(p[0].ptr == p[1].ptr && p[0].stride == p[1].stride) &&
            !ksp_planes_apart(p[0], rows, cols, p[1], rows, cols)) {
            ksp_set_error("invalid argument: %s overlaps %s without being %s with the same stride",
                          p[1].name, p[0].name, p[0].name);
            return (int)hipErrorInvalidValue;
        }
    return 0;
}

// The grid of a kernel whose threads each take a run of `run` adjacent columns of one row,
// runs numbered row by row: `groups` workgroups of `threads`.
struct ksp_run_grid {
    int runs_per_row;
    long long runs, groups;
};
inline int ksp_make_run_grid(long long rows, int cols, int run, int threads, ksp_run_grid &g)
{
    g.runs_per_row = (int)(((long long)cols + run - 1) / run);
    g.runs = rows * g.runs_per_row;
    g.groups = (g.runs + threads - 1) / threads;
    if (g.groups > 0x7fffffffll) {
        ksp_set_error("invalid argument: array too large for one launch");
        return (int)hipErrorInvalidValue;
    }
    return 0;
}

// One value per device, for what is set up or queried once per device: T() means "not yet".
// A device outside 0 .. 63 has no slot: get() says "not yet" every time and set() does
// nothing, so its caller does the work on every call. Static storage (zero-initialised).
template <typename T>
struct KspPerDevice {
    std::atomic<T> slot[64];
    static bool has_slot(int device) { return device >= 0 && device < 64; }
    T get(int device) const
    {
        return has_slot(device) ? slot[device].load(std::memory_order_acquire) : T();
    }
    void set(int device, T value)
    {
        if (has_slot(device)) slot[device].store(value, std::memory_order_release);
    }
};

// The opt-in of Kernel to `bytes` of dynamic LDS (more than the default 64 KiB), once per
// device: one context per device in one process is a supported arrangement (reference
// doc/user/init.rst:4-6). `did` (optional) is told whether this call was the one.
template <auto Kernel>
inline int ksp_lds_opt_in(int device, size_t bytes, bool *did = nullptr)
{
    static KspPerDevice<bool> done;
    if (did != nullptr) *did = !done.get(device);
    if (done.get(device)) return 0;
    KSP_CHECK(hipFuncSetAttribute((const void *)Kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.set(device, true);
    return 0;
}

// Launch with the events of ksp_flagger_fused_profile around the kernel itself (not around
// a zero fill before it) when they are armed, a plain launch otherwise.
template <typename K, typename... Args>
inline int ksp_launch_timed(K kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s,
                            hipEvent_t ev0, hipEvent_t ev1, const Args &...args)
{
    if (ev0 != nullptr)
        hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, s, ev0, ev1, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
    KSP_LAUNCH_CHECK();
    return 0;
}
