// The run of the streaming kernels, and how it moves between memory and registers. Device code
// only; include it after ksp_common.h.
//
// Layout. The arrays are [rows][stride] with the columns contiguous, and a lane owns a run of
// KSP_RUN = 16 adjacent columns of one row: 16 flag bytes are one 16-byte access, 16 floats
// four, 16 complex values eight. A run whose `valid` columns (counted from its first to the
// end of the row; may be <= 0) are all there moves with 16-byte accesses when the caller says
// `wide`: every pointer and every row start of the array is a multiple of 16 bytes
// (ksp_rows_aligned). The ragged run at the end of a row, and every run of an array that is not
// aligned so, goes element by element and touches only elements inside the row: padding is
// neither read nor written, and `valid <= 0` dereferences nothing.
//
// A kernel loads a run into a register array, states its arithmetic once over the KSP_RUN
// elements, and stores the result; elements beyond `valid` hold a fill value that is computed
// with and dropped. `wide` is an ordinary bool: where it is a constant at the call site, the
// other path folds away.
//
// compress_weights.hip, flag_count.hip, apply_gains.hip, predict.hip and the row pass of sir.hip
// are written on these helpers. average.hip and prepare.hip have the same layout but hold several
// arrays of a run at once, and keep their own two paths (profiles/run16.md).
#pragma once

#define KSP_RUN 16

// 16 bytes as one access. Flag bytes stay packed like this: byte i of a run is bits
// 8 (i % 4) .. 8 (i % 4) + 7 of word i / 4.
typedef unsigned ksp_run_bytes __attribute__((ext_vector_type(4)));

// The elements of a run (T: a 4- or 8-byte type such as float, int, float2); those at and
// beyond `valid` read as `fill`.
template <typename T>
__device__ __forceinline__ void ksp_run_load(const T *p, int valid, bool wide, T (&v)[KSP_RUN],
                                             T fill)
{
    if (wide && valid >= KSP_RUN) {
#pragma unroll
        for (int q = 0; q < (int)sizeof(v) / 16; q++) {
            const ksp_run_bytes t = reinterpret_cast<const ksp_run_bytes *>(p)[q];
            __builtin_memcpy(&v[q * (16 / sizeof(T))], &t, 16);
        }
    } else {
#pragma unroll
        for (int i = 0; i < KSP_RUN; i++) v[i] = i < valid ? T(p[i]) : fill;
    }
}

// The other way: the first `valid` elements of a run are stored, the rest dropped.
template <typename T>
__device__ __forceinline__ void ksp_run_store(T *p, int valid, bool wide, const T (&v)[KSP_RUN])
{
    if (wide && valid >= KSP_RUN) {
#pragma unroll
        for (int q = 0; q < (int)sizeof(v) / 16; q++) {
            ksp_run_bytes t;
            __builtin_memcpy(&t, &v[q * (16 / sizeof(T))], 16);
            reinterpret_cast<ksp_run_bytes *>(p)[q] = t;
        }
    } else {
#pragma unroll
        for (int i = 0; i < KSP_RUN; i++)
            if (i < valid) p[i] = v[i];
    }
}

// The flag bytes of a run; bytes at and beyond `valid` read as zero and are not stored.
__device__ __forceinline__ ksp_run_bytes ksp_run_load_bytes(const uint8_t *p, int valid, bool wide)
{
    if (wide && valid >= KSP_RUN) return *reinterpret_cast<const ksp_run_bytes *>(p);
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < KSP_RUN; i++)
        if (i < valid) w[i / 4] |= (unsigned)p[i] << (8 * (i % 4));
    return ksp_run_bytes{w[0], w[1], w[2], w[3]};
}

// f[i] |= flag_value for every element i of the run whose bit of `bad` is set.
__device__ __forceinline__ void ksp_flag_spread(ksp_run_bytes &f, unsigned bad, unsigned flag_value)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        // bit k of the nibble to bit 0 of byte k (no two products share a bit)
        const unsigned spread = (((bad >> (4 * q)) & 0xfu) * 0x00204081u) & 0x01010101u;
        f[q] |= spread * flag_value;
    }
}

__device__ __forceinline__ void ksp_run_store_bytes(uint8_t *p, int valid, bool wide,
                                                    ksp_run_bytes w)
{
    if (wide && valid >= KSP_RUN) {
        *reinterpret_cast<ksp_run_bytes *>(p) = w;
        return;
    }
#pragma unroll
    for (int i = 0; i < KSP_RUN; i++)
        if (i < valid) p[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}
