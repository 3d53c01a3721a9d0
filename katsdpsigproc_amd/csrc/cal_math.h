// Device arithmetic the calibration kernels share (apply_gains, solve_gains, solve_jones, predict,
// fit_delays, interpolate_gains, interpolate_jones). Each kernel reproduces a host class of
// rfi/host.py bit for bit, so every helper is one float operation per written step, in the order
// written, with intrinsics that are never contracted; a helper stands only where a kernel's
// expression is operation for operation this one. Device code only.
#pragma once
#include "ksp_common.h"

// ---- complex float32 (host: _product and the expressions around it)

// a b
__device__ __forceinline__ float2 ksp_cmul(float2 a, float2 b)
{
    return make_float2(__fsub_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)),
                       __fadd_rn(__fmul_rn(a.x, b.y), __fmul_rn(a.y, b.x)));
}

// a conj(b)
__device__ __forceinline__ float2 ksp_cmul_conj(float2 a, float2 b)
{
    return make_float2(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)),
                       __fsub_rn(__fmul_rn(a.y, b.x), __fmul_rn(a.x, b.y)));
}

// re re + im im
__device__ __forceinline__ float ksp_norm2(float2 a)
{
    return __fadd_rn(__fmul_rn(a.x, a.x), __fmul_rn(a.y, a.y));
}

__device__ __forceinline__ bool ksp_cfinite(float2 a)
{
    return __builtin_isfinite(a.x) && __builtin_isfinite(a.y);
}

// q = re re + im im;  q > 0 ? (re / q, -im / q) : NaN   (a NaN q is not above 0)
__device__ __forceinline__ float2 ksp_creciprocal_or_nan(float2 a)
{
    const float q = ksp_norm2(a);
    const float nan32 = __builtin_nanf("");
    return q > 0.0f ? make_float2(__fdiv_rn(a.x, q), __fdiv_rn(-a.y, q))
                    : make_float2(nan32, nan32);
}

// ---- 2x2 complex float32 (host: SolveJonesHost; a matrix is [[a, b], [c, d]])

// a + b,  a - b
__device__ __forceinline__ float2 ksp_cadd(float2 a, float2 b)
{
    return make_float2(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y));
}
__device__ __forceinline__ float2 ksp_csub(float2 a, float2 b)
{
    return make_float2(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y));
}

// the determinant a d - b c
__device__ __forceinline__ float2 ksp_det2(float2 a, float2 b, float2 c, float2 d)
{
    return ksp_csub(ksp_cmul(a, d), ksp_cmul(b, c));
}

// (x, y) . conj((u, v)) = x conj(u) + y conj(v): a row times the conjugate of another
__device__ __forceinline__ float2 ksp_row_dot_conj(float2 x, float2 y, float2 u, float2 v)
{
    return ksp_cadd(ksp_cmul_conj(x, u), ksp_cmul_conj(y, v));
}

// row `odd` of the adjugate [[d, -b], [-c, a]] times the scalar i: (d i, -(b i)) or
// (-(c i), a i); the product is negated, not the factor (the sign of a zero differs)
__device__ __forceinline__ void ksp_adj2_row_times(float2 a, float2 b, float2 c, float2 d,
                                                   float2 i, bool odd, float2 &first,
                                                   float2 &second)
{
    const float2 keep = ksp_cmul(odd ? a : d, i), turn = ksp_cmul(odd ? c : b, i);
    const float2 minus = make_float2(-turn.x, -turn.y);
    first = odd ? minus : keep;
    second = odd ? keep : minus;
}

// ---- float64 (host: PredictHost.cos_sin)

// (cos, sin) of 2 pi x, x in turns:
//   r  = x - rint(x);  q = rint(4 * r);  y = r - q * 0.25;  z = y * 6.283185307179586
//   z2 = z * z
//   sn = (((((S5*z2 + S4)*z2 + S3)*z2 + S2)*z2 + S1)*z2 + S0) * z
//   cs = (((((C6*z2 + C5)*z2 + C4)*z2 + C3)*z2 + C2)*z2 + C1)*z2 + C0
//     S0..S5 = 1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984,
//              2.7557319223985893e-06, -2.505210838544172e-08
//     C0..C6 = 1.0, -0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05,
//              -2.755731922398589e-07, 2.08767569878681e-09
//   (co, si) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)   for q = 0, 1, +-2, -1
__device__ __forceinline__ void ksp_cos_sin_turns(double x, double &co, double &si)
{
    const double r = __dsub_rn(x, rint(x));
    const double q = rint(__dmul_rn(4.0, r));
    const double y = __dsub_rn(r, __dmul_rn(q, 0.25));
    const double z = __dmul_rn(y, 6.283185307179586);
    const double z2 = __dmul_rn(z, z);
    double sn = -2.505210838544172e-08;
    sn = __dadd_rn(__dmul_rn(sn, z2), 2.7557319223985893e-06);
    sn = __dadd_rn(__dmul_rn(sn, z2), -0.0001984126984126984);
    sn = __dadd_rn(__dmul_rn(sn, z2), 0.008333333333333333);
    sn = __dadd_rn(__dmul_rn(sn, z2), -0.16666666666666666);
    sn = __dadd_rn(__dmul_rn(sn, z2), 1.0);
    sn = __dmul_rn(sn, z);
    double cs = 2.08767569878681e-09;
    cs = __dadd_rn(__dmul_rn(cs, z2), -2.755731922398589e-07);
    cs = __dadd_rn(__dmul_rn(cs, z2), 2.48015873015873e-05);
    cs = __dadd_rn(__dmul_rn(cs, z2), -0.001388888888888889);
    cs = __dadd_rn(__dmul_rn(cs, z2), 0.041666666666666664);
    cs = __dadd_rn(__dmul_rn(cs, z2), -0.5);
    cs = __dadd_rn(__dmul_rn(cs, z2), 1.0);
    // q is -2 .. 2, or NaN, which takes the first row of the table with NaN in both
    const bool odd = q == 1.0 || q == -1.0, half = q == 2.0 || q == -2.0;
    co = odd ? sn : cs;
    si = odd ? cs : sn;
    co = q == 1.0 || half ? -co : co;
    si = q == -1.0 || half ? -si : si;
}
