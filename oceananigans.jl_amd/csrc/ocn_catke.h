// ocn_catke.h -- the scalar functions of CATKEVerticalDiffusivity that must give the same bits on the device, on the host and in
// tests/catke_numpy.py: Julia's min / max / Bool multiplication and a cube root.  __host__ __device__ functions made of IEEE +, -, *, /,
// comparisons and exponent manipulation, built in the strict set (-ffp-contract=off), in the style of ocn_taper.h.
#pragma once
#include <cstdint>
#include <cstring>

#ifndef __host__  // a plain C++ compiler (a host-only build of this header under a sanitizer) knows no execution-space qualifiers
#define __host__
#define __device__
#endif

namespace ocn {

namespace catke {

__host__ __device__ inline uint64_t bits_of(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return b;
}
__host__ __device__ inline double from_bits(uint64_t b)
{
    double x;
    __builtin_memcpy(&x, &b, sizeof x);
    return x;
}
__host__ __device__ inline bool sign_of(double x) { return (bits_of(x) >> 63) != 0; }

// Julia's max(a, b) / min(a, b) of Float64: a NaN propagates, max(0.0, -0.0) = 0.0, min(0.0, -0.0) = -0.0
__host__ __device__ inline double jmax(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a > b) return a;
    if (b > a) return b;
    return sign_of(a) ? b : a;
}
__host__ __device__ inline double jmin(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a < b) return a;
    if (b < a) return b;
    return sign_of(a) ? a : b;
}
__host__ __device__ inline double clip(double x) { return jmax(0.0, x); }

// Julia's x * flag for a Bool flag (base/bool.jl): false is a "strong zero", x * false = copysign(0, x) even for an infinite x.  For a
// NaN x Julia's result carries the NaN's sign bit, which differs between machines for the same 0 / 0: +0 here (tests/catke_numpy.py too).
__host__ __device__ inline double bmul(double x, bool flag)
{
    if (flag) return x;
    if (x != x) return 0.0;
    return sign_of(x) ? -0.0 : 0.0;
}

// 2^k for -1022 <= k <= 1023, from its bits
__host__ __device__ inline double pow2(int k) { return from_bits((uint64_t)(k + 1023) << 52); }

// cbrt(x).  No cbrt is correctly rounded, and libm, the device library and NumPy differ in the last bit, so this one is written out:
//   ±0, ±inf and NaN come back as they are;  |x| = m 2^e, 1 <= m < 2 (a subnormal is first scaled by 2^54, the result by 2^-18);
//   e = 3 q + r, r in {0, 1, 2};  a = m 2^r in [1, 8);  y0 = 1 + (a - 1) / 7 (the chord of the cube root over [1, 8]: at most 11 % too
//   small);  six Newton steps y <- (2 y + a / (y y)) / 3 (the relative error squares: 1.1e-1, 1.3e-2, 1.7e-4, 2.9e-8, 8e-16, rounding);
//   cbrt(x) = ±y 2^q, an exact scaling.  The measured distance to a correctly rounded cube root: DESIGN.md §5.2o.
__host__ __device__ inline double cbrt_newton(double x)
{
    if (x != x || x == 0.0) return x;
    const bool negative = sign_of(x);
    double a = negative ? -x : x;
    if (a > 1.7976931348623157e308) return x;
    int post = 0;
    if (a < 2.2250738585072014e-308) {  // subnormal: 2^54 = (2^18)^3
        a = a * 18014398509481984.0;
        post = -18;
    }
    const uint64_t b = bits_of(a);
    const int e = (int)((b >> 52) & 0x7ff) - 1023;
    const int q = e >= 0 ? e / 3 : -((-e + 2) / 3);
    const int r = e - 3 * q;
    const double m = from_bits((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);
    a = m * pow2(r);
    double y = 1.0 + (a - 1.0) / 7.0;
    for (int n = 0; n < 6; ++n) y = (2.0 * y + a / (y * y)) / 3.0;
    y = y * pow2(q + post);
    return negative ? -y : y;
}

}  // namespace catke

}  // namespace ocn
