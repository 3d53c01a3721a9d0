// Work-group reductions for run-time compiled kernels (HIP, gfx950).
//
// Counterpart of the reference's wg_reduce.mako (define_scratch / define_function, its
// lines 71-96 give the contract): SIZE cooperating work-items combine one value each
// with a commutative, associative operator. Where the reference generates one struct and
// one function per use from Mako defs, this header has one scratch template and one
// function template:
//
//     LOCAL_DECL ksp::wg_reduce_scratch<float, 256, true> scratch;
//     float total = ksp::wg_reduce<float, 256, ksp::op_plus, false, true>(
//         value, get_local_id(0), &scratch);
//
// Contract
//  * Every work-item of the work-group calls wg_reduce, without divergence: the function
//    contains barriers (except in the one case noted below).
//  * The work-group may be partitioned into sets of SIZE work-items; each set passes its
//    own scratch instance and an idx in 0..SIZE-1.
//  * BROADCAST false: only idx 0 holds a defined result.
//  * SHUFFLE true is the caller's promise that idx is the linear work-item id modulo
//    SIZE. A set then occupies whole, aligned runs of lanes of the 64-wide wavefronts,
//    and when SIZE is a power of two or a multiple of 64 the lanes of a wavefront
//    exchange values over DPP and ds_bpermute; sets wider than a wavefront combine one
//    LDS word per wavefront. For SIZE <= 64 that path has no barrier and the scratch has
//    no data at all.
//  * SHUFFLE false, or any other SIZE: nothing is assumed about which wavefront holds
//    which idx; values travel through LDS between barriers only.
//  * The scratch may be reused by the next reduction straight away: every path that
//    touches it ends on a barrier.
//
// The value type is any trivially copyable type whose size is a multiple of 4 bytes and
// which the operator accepts (int, unsigned, long long, float, double, float2, ...).
#pragma once
#include "port.h"

namespace ksp
{

// ------------------------------------------------------------------------- operators
namespace detail
{
template <class A, class B> struct same_type { static constexpr bool value = false; };
template <class A> struct same_type<A, A> { static constexpr bool value = true; };
}  // namespace detail

struct op_plus
{
    template <class T> DEVICE_FN T operator()(T a, T b) const { return a + b; }
};
struct op_min
{
    template <class T> DEVICE_FN T operator()(T a, T b) const { return b < a ? b : a; }
};
struct op_max
{
    template <class T> DEVICE_FN T operator()(T a, T b) const { return a < b ? b : a; }
};
// fmin / fmax ignore NaN on float and double (the result is NaN only when both sides
// are); on every other type they are min / max
struct op_fmin
{
    template <class T> DEVICE_FN T operator()(T a, T b) const
    {
        if constexpr (detail::same_type<T, float>::value)
            return __builtin_fminf(a, b);
        else if constexpr (detail::same_type<T, double>::value)
            return __builtin_fmin(a, b);
        else
            return b < a ? b : a;
    }
};
struct op_fmax
{
    template <class T> DEVICE_FN T operator()(T a, T b) const
    {
        if constexpr (detail::same_type<T, float>::value)
            return __builtin_fmaxf(a, b);
        else if constexpr (detail::same_type<T, double>::value)
            return __builtin_fmax(a, b);
        else
            return a < b ? b : a;
    }
};

// ------------------------------------------------------------------------- internals
namespace detail
{
constexpr int WAVE = KSP_SIMD_GROUP_SIZE;

constexpr bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
constexpr bool use_shuffle(int size, bool shuffle)
{
    return shuffle && (is_pow2(size) || size % WAVE == 0);
}
// elements of LDS a reduction needs
constexpr int scratch_elements(int size, bool shuffle)
{
    return use_shuffle(size, shuffle) ? (size <= WAVE ? 0 : size / WAVE) : size;
}

template <class T, int N> struct scratch_storage
{
    T data[N];
};
template <class T> struct scratch_storage<T, 0>
{
};

// DPP controls: the partner of lane l is l ^ 1, l ^ 2 (quad_perm), 7 - (l % 8) + 8 * (l / 8)
// (row_half_mirror) and 15 - (l % 16) + 16 * (l / 16) (row_mirror). Once the quads hold one
// value each, the mirrors pair every lane with a lane of the other quad / other half row,
// which is all a commutative butterfly needs.
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

template <int CTRL> DEVICE_FN int dpp_word(int w)
{
    return __builtin_amdgcn_update_dpp(w, w, CTRL, 0xf, 0xf, false);
}

// value of the partner lane at butterfly distance OFF (1, 2, 4, ... 32), word by word
template <int OFF, class T> DEVICE_FN T butterfly_partner(const T &value)
{
    static_assert(sizeof(T) % 4 == 0, "wg_reduce: the value's size must be a multiple of 4 bytes");
    constexpr int WORDS = sizeof(T) / 4;
    int w[WORDS];
    __builtin_memcpy(w, &value, sizeof(T));
#pragma unroll
    for (int i = 0; i < WORDS; i++) {
        if constexpr (OFF == 1)
            w[i] = dpp_word<DPP_XOR1>(w[i]);
        else if constexpr (OFF == 2)
            w[i] = dpp_word<DPP_XOR2>(w[i]);
        else if constexpr (OFF == 4)
            w[i] = dpp_word<DPP_HALF_MIRROR>(w[i]);
        else if constexpr (OFF == 8)
            w[i] = dpp_word<DPP_MIRROR>(w[i]);
        else
            w[i] = __shfl_xor(w[i], OFF, WAVE);
    }
    T other;
    __builtin_memcpy(&other, w, sizeof(T));
    return other;
}

// Combine the values of aligned runs of LANES lanes (a power of two <= 64); every lane of
// a run ends up with the run's result.
template <int LANES, int OFF = 1, class T, class Op> DEVICE_FN T lanes_reduce(T value, Op op)
{
    if constexpr (OFF < LANES) {
        value = op(value, butterfly_partner<OFF>(value));
        return lanes_reduce<LANES, OFF * 2>(value, op);
    } else
        return value;
}
}  // namespace detail

// --------------------------------------------------------------------------- scratch
/// LDS for one set of SIZE cooperating work-items (declare it LOCAL_DECL). SHUFFLE must
/// match the wg_reduce call that uses it.
template <class T, int SIZE, bool SHUFFLE = false>
struct wg_reduce_scratch : detail::scratch_storage<T, detail::scratch_elements(SIZE, SHUFFLE)>
{
    static_assert(SIZE >= 1 && SIZE <= 1024, "wg_reduce: SIZE must be in 1..1024");
};

// ---------------------------------------------------------------------------- reduce
template <class T, int SIZE, class Op = op_plus, bool BROADCAST = true, bool SHUFFLE = false>
DEVICE_FN T wg_reduce(T value, int idx, LOCAL wg_reduce_scratch<T, SIZE, SHUFFLE> *scratch,
                      Op op = Op())
{
    using namespace detail;
    if constexpr (SIZE == 1) {
        return value;
    } else if constexpr (use_shuffle(SIZE, SHUFFLE) && SIZE <= WAVE) {
        // the set is an aligned run of SIZE lanes of one wavefront
        return lanes_reduce<SIZE>(value, op);
    } else if constexpr (use_shuffle(SIZE, SHUFFLE)) {
        // the set is SIZE / 64 whole wavefronts: one LDS word for each
        constexpr int WAVES = SIZE / WAVE;
        value = lanes_reduce<WAVE>(value, op);
        if ((idx & (WAVE - 1)) == 0) scratch->data[idx / WAVE] = value;
        BARRIER();
        if (BROADCAST || idx < WAVE) {  // uniform over a wavefront
            value = scratch->data[0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) value = op(value, scratch->data[w]);
        }
        BARRIER();  // the caller may write to the scratch again at once
        return value;
    } else {
        // LDS only. The first RAKE work-items each fold a strided share of the rest, then
        // a tree halves the survivors; an idx may sit in any wavefront, so every step is
        // fenced by a work-group barrier that all work-items reach.
        constexpr int RAKE = SIZE < WAVE ? SIZE : WAVE;
        if constexpr (SIZE > RAKE) {
            if (idx >= RAKE) scratch->data[idx] = value;
            BARRIER();
        }
        if (idx < RAKE) {
            for (int i = idx + RAKE; i < SIZE; i += RAKE) value = op(value, scratch->data[i]);
            scratch->data[idx] = value;
        }
#pragma unroll
        for (int n = RAKE; n > 1; n = (n + 1) / 2) {
            const int half = (n + 1) / 2;  // data[0 .. n) is live; fold [half, n) onto [0, n / 2)
            BARRIER();
            if (idx < n / 2) {
                value = op(value, scratch->data[idx + half]);
                scratch->data[idx] = value;
            }
        }
        if constexpr (BROADCAST) {
            BARRIER();
            value = scratch->data[0];
        }
        BARRIER();  // the caller may write to the scratch again at once
        return value;
    }
}

}  // namespace ksp
