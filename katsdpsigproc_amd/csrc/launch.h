// Host-side launch helpers: a run-time integer as a template argument, the alignment test of
// the 16-byte load paths, what a launcher does once per device, and the choice between a
// plain and an event-timed launch. No device code.
#pragma once
#include <hip/hip_ext.h>

#include <atomic>
#include <type_traits>

#include "ksp_common.h"

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

// Whether rows that start at `ptr` and lie `stride` elements of `elem_bytes` bytes apart can
// be read in pieces of `bytes` bytes: every row starts on a multiple of `bytes`.
inline bool ksp_rows_aligned(const void *ptr, long long stride, int elem_bytes, int bytes = 16)
{
    return (uintptr_t)ptr % bytes == 0 && stride * elem_bytes % bytes == 0;
}

// The same for an optional array: one that is not given (NULL) does not object.
inline bool ksp_rows_aligned_if_given(const void *ptr, long long stride, int elem_bytes)
{
    return ptr == nullptr || ksp_rows_aligned(ptr, stride, elem_bytes);
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
