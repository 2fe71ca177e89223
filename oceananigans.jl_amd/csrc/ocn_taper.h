// ocn_taper.h -- the Ri-dependent tapering functions of RiBasedVerticalDiffusivity (ri_based_vertical_diffusivity.jl:239-241)
//
//   Linear: 1 - min(1, max(0, (x - x₀) / δ))      Exp: exp(-max(0, (x - x₀) / δ))      Tanh: (1 - tanh((x - x₀) / δ)) / 2
//
// as __host__ __device__ functions made of IEEE +, -, *, /, comparisons, the exact conversion of an integer-valued double and exact scaling
// by powers of two -- no call into a math library, whose exp / tanh differ between the device, libm and NumPy.  Built in the strict set
// (-ffp-contract=off: no FMA), so the device, ocn_ri_taper_host and tests/ri_based_numpy.py give the same bits.  min / max propagate a NaN
// as Julia's do.  Accuracy against an extended-precision evaluation of the formulas above: DESIGN.md §5.2k.
#pragma once
#include <cstdint>
#include <cstring>

#ifndef __host__  // a plain C++ compiler (a host-only build of this header under a sanitizer) knows no execution-space qualifiers
#define __host__
#define __device__
#endif

namespace ocn {

namespace taper {

// 2^k for -1022 <= k <= 1023, from its bits
__host__ __device__ inline double pow2(int k)
{
    const uint64_t bits = (uint64_t)(k + 1023) << 52;
    double s;
    memcpy(&s, &bits, sizeof s);
    return s;
}

// exp(x) for x <= 0 (the only arguments the tapers have); a NaN comes back as it is; x < -746 (exp(x) < 2^-1076, -inf included) gives 0.
//   k = the integer nearest to x / ln 2, by adding and subtracting 1.5 * 2^52 (round to nearest even; |x / ln 2| < 2^11)
//   r = (x - k LN2_HI) - k LN2_LO: LN2_HI holds the leading 32 bits of ln 2, so k LN2_HI is exact; |r| <= 0.3466 (plus 1e-13)
//   exp(r) = Σ r^n / n!, n = 0..13, by Horner's rule: the first term left out is below 0.3466^14 / 14! = 4.1e-18 < 2^-57
//   exp(x) = exp(r) 2^k, in two exact steps 2^-h, 2^(k + h), h = -k / 2 -- the second one rounds, once, where the result is subnormal.
__host__ __device__ inline double exp_nonpositive(double x)
{
    constexpr double INV_LN2 = 1.4426950408889634, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    constexpr double MAGIC = 6755399441055744.0;  // 1.5 * 2^52
    if (x != x) return x;
    if (x < -746.0) return 0.0;
    const double kd = (x * INV_LN2 + MAGIC) - MAGIC;
    const double r = (x - kd * LN2_HI) - kd * LN2_LO;
    double p = 1.0 / 6227020800.0;                 // 1 / 13!
    p = 1.0 / 479001600.0 + r * p;                 // 1 / 12!
    p = 1.0 / 39916800.0 + r * p;
    p = 1.0 / 3628800.0 + r * p;
    p = 1.0 / 362880.0 + r * p;
    p = 1.0 / 40320.0 + r * p;
    p = 1.0 / 5040.0 + r * p;
    p = 1.0 / 720.0 + r * p;
    p = 1.0 / 120.0 + r * p;
    p = 1.0 / 24.0 + r * p;
    p = 1.0 / 6.0 + r * p;
    p = 0.5 + r * p;
    p = 1.0 + r * p;
    p = 1.0 + r * p;
    const int k = (int)kd, h = (-k) / 2;  // k <= 0
    return (p * pow2(-h)) * pow2(k + h);
}

// tanh(x) = ±(1 - e) / (1 + e), e = exp(-2 |x|); ±1 for |x| > 20 (1 - tanh 20 = 8.5e-18 < 2^-54), ±inf included; a NaN comes back as it is.
// The ABSOLUTE error is what the taper needs and what is bounded; next to 0 the subtraction 1 - e loses the relative accuracy.
__host__ __device__ inline double tanh_absolute(double x)
{
    const double a = x < 0 ? -x : x;
    if (a > 20.0) return x < 0 ? -1.0 : 1.0;
    const double e = exp_nonpositive(-(2.0 * a));
    const double t = (1.0 - e) / (1.0 + e);
    return x < 0 ? -t : t;
}

// Julia's max(0, q) and min(1, q): a NaN propagates
__host__ __device__ inline double max_zero(double q) { return q != q ? q : (q > 0.0 ? q : 0.0); }
__host__ __device__ inline double min_one(double q) { return q != q ? q : (q < 1.0 ? q : 1.0); }

__host__ __device__ inline double linear(double x, double x0, double delta) { return 1.0 - min_one(max_zero((x - x0) / delta)); }
__host__ __device__ inline double exponential(double x, double x0, double delta) { return exp_nonpositive(-max_zero((x - x0) / delta)); }
__host__ __device__ inline double hyperbolic_tangent(double x, double x0, double delta)
{
    return (1.0 - tanh_absolute((x - x0) / delta)) / 2.0;
}

// kind: OCN_RI_TAPER_LINEAR / EXP / TANH (include/ocn_hip.h), validated by the callers
__host__ __device__ inline double apply(int kind, double x, double x0, double delta)
{
    if (kind == 0) return linear(x, x0, delta);
    if (kind == 1) return exponential(x, x0, delta);
    return hyperbolic_tangent(x, x0, delta);
}

}  // namespace taper

}  // namespace ocn
