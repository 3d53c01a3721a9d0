// Rank statistics for run-time compiled kernels (HIP, gfx950).
//
// Counterpart of the reference's rank.mako. A *ranker* answers four questions about a
// set of values:
//
//     zeros()          how many are equal to zero
//     rank(v)          how many are strictly below v (NaN is never counted; v not NaN)
//     fmin() / fmax()  the smallest / largest non-NaN value, NaN if there is none
//     max_below(lim)   the largest non-NaN value strictly below lim, 0 if there is none
//
// Three rankers are provided:
//
//   ranker_serial<T, Foreach>          one work-item walks the values itself; the caller
//                                      supplies the walk as `foreach(body)`, which calls
//                                      body(value) for each one (make_ranker_serial<T>
//                                      deduces the lambda's type)
//   ranker_serial_store<T, N>          the same over N values kept in registers, which
//                                      the caller fills and pads with NaN
//   ranker_parallel<Serial, T, SIZE>   SIZE work-items, each with a serial ranker over
//                                      its share, answer collectively through
//                                      wg_reduce.h; every answer is broadcast
//
// On top of any ranker over positive 32-bit floats: find_rank_float (the value of a
// given rank, by a search on the bit pattern, which for positive floats orders like the
// value), find_min_float, find_max_float and median_non_zero_float. Their UNIFORM switch
// says whether the whole work-group works on one data set with the same arguments
// (true), or each work-item or set of work-items on its own (false): only with UNIFORM
// may a collective ranker be called under a condition.
#pragma once
#include "port.h"
#include "wg_reduce.h"

namespace ksp
{

// ---------------------------------------------------------------------------- serial
template <class T, class Foreach> struct ranker_serial
{
    Foreach foreach;

    DEVICE_FN explicit ranker_serial(Foreach f) : foreach(f) {}

    DEVICE_FN int zeros() const
    {
        int n = 0;
        foreach([&](T v) { n += v == T(0); });
        return n;
    }

    DEVICE_FN int rank(T value) const
    {
        int n = 0;
        foreach([&](T v) { n += v < value; });
        return n;
    }

    DEVICE_FN T fmin() const { return fold(op_fmin()); }
    DEVICE_FN T fmax() const { return fold(op_fmax()); }

    DEVICE_FN T max_below(T limit) const
    {
        T best = T(0);
        foreach([&](T v) {
            if (v > best && v < limit) best = v;
        });
        return best;
    }

private:
    // the walk must not be empty: the first value seeds the fold
    template <class Op> DEVICE_FN T fold(Op op) const
    {
        T acc = T();
        bool seeded = false;
        foreach([&](T v) {
            acc = seeded ? op(acc, v) : v;
            seeded = true;
        });
        return acc;
    }
};

template <class T, class Foreach> DEVICE_FN ranker_serial<T, Foreach> make_ranker_serial(Foreach f)
{
    return ranker_serial<T, Foreach>(f);
}

namespace detail
{
template <class T, int N> struct stored_values
{
    T values[N];
    template <class Body> DEVICE_FN void operator()(Body &&body) const
    {
#pragma unroll
        for (int i = 0; i < N; i++) body(values[i]);
    }
};
}  // namespace detail

/// Serial ranker over N values of its own, which the caller fills through `ranker[i]`;
/// unused places hold NaN.
template <class T, int N> struct ranker_serial_store : ranker_serial<T, detail::stored_values<T, N>>
{
    DEVICE_FN ranker_serial_store()
        : ranker_serial<T, detail::stored_values<T, N>>(detail::stored_values<T, N>())
    {
    }
    DEVICE_FN T &operator[](int i) { return this->foreach.values[i]; }
    DEVICE_FN const T &operator[](int i) const { return this->foreach.values[i]; }
};

// -------------------------------------------------------------------------- parallel
/// LDS of one ranker_parallel: its counts and its extremes are never live together.
template <class T, int SIZE, bool SHUFFLE = false> union ranker_parallel_scratch
{
    wg_reduce_scratch<int, SIZE, SHUFFLE> sum;
    wg_reduce_scratch<T, SIZE, SHUFFLE> minmax;
};

/// The serial interface, collective over SIZE work-items: `serial` covers this
/// work-item's share, `idx` is its place 0..SIZE-1 in the set and `scratch` the set's
/// LDS. Every work-item of the work-group must make each call, as for wg_reduce, and
/// SHUFFLE carries the same promise about idx.
template <class Serial, class T, int SIZE, bool SHUFFLE = false> struct ranker_parallel
{
    typedef ranker_parallel_scratch<T, SIZE, SHUFFLE> scratch_type;

    Serial &serial;
    LOCAL scratch_type *scratch;
    int idx;

    DEVICE_FN ranker_parallel(Serial &serial, LOCAL scratch_type *scratch, int idx)
        : serial(serial), scratch(scratch), idx(idx)
    {
    }

    DEVICE_FN int zeros() const { return sum(serial.zeros()); }
    DEVICE_FN int rank(T value) const { return sum(serial.rank(value)); }
    DEVICE_FN T fmin() const
    {
        return wg_reduce<T, SIZE, op_fmin, true, SHUFFLE>(serial.fmin(), idx, &scratch->minmax);
    }
    DEVICE_FN T fmax() const
    {
        return wg_reduce<T, SIZE, op_fmax, true, SHUFFLE>(serial.fmax(), idx, &scratch->minmax);
    }
    DEVICE_FN T max_below(T limit) const
    {
        return wg_reduce<T, SIZE, op_fmax, true, SHUFFLE>(serial.max_below(limit), idx,
                                                          &scratch->minmax);
    }

private:
    DEVICE_FN int sum(int n) const
    {
        return wg_reduce<int, SIZE, op_plus, true, SHUFFLE>(n, idx, &scratch->sum);
    }
};

// ------------------------------------------------------------ positive 32-bit floats
/// The value of rank `rank` (0 is the smallest); with `halfway`, the float32 mean of
/// ranks `rank` and `rank - 1`. The values must be positive floats (zeros allowed).
template <bool UNIFORM, class Ranker>
DEVICE_FN float find_rank_float(const Ranker &ranker, int rank, bool halfway)
{
    // grow the bit pattern from the top: a bit stays when no more than `rank` values lie
    // below the candidate, which ends on the largest pattern with that property
    unsigned bits = 0;
    for (unsigned bit = 1u << 30; bit != 0; bit >>= 1)
        if (ranker.rank(as_float(bits | bit)) <= rank) bits |= bit;
    float result = as_float(bits);
    if constexpr (UNIFORM) {
        // exactly `rank` values below: rank - 1 is a smaller value, the next one down
        if (halfway && ranker.rank(result) == rank)
            result = (result + ranker.max_below(result)) * 0.5f;
    } else {
        // the ranker may hold barriers, which not every work-item would reach inside the
        // condition
        const int below = ranker.rank(result);
        const float prev = ranker.max_below(result);
        if (halfway && below == rank) result = (result + prev) * 0.5f;
    }
    return result;
}

template <class Ranker> DEVICE_FN float find_min_float(const Ranker &ranker)
{
    return ranker.fmin();
}

template <class Ranker> DEVICE_FN float find_max_float(const Ranker &ranker)
{
    return ranker.fmax();
}

/// Median of the non-zero values among the ranker's `n` (NaN padding not counted in n).
/// Undefined when n is zero or every value is.
template <bool UNIFORM, class Ranker>
DEVICE_FN float median_non_zero_float(const Ranker &ranker, int n)
{
    const int twice = n + ranker.zeros();  // twice the median's rank among all n
    return find_rank_float<UNIFORM>(ranker, twice / 2, !(twice & 1));
}

}  // namespace ksp
