// lk_host.h -- host-side arithmetic of the LK launch that a program without HIP can include (tests/native/lk_bound_harness.cpp).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

// The division-free form of `fl(x / den) < t` for a positive finite float den: the float X with
//     fl(x / den) < t   <=>   x < X          for EVERY float x (NaN included: both sides are false),
// where fl(x / den) is the correctly rounded (IEEE-754, round to nearest even) float quotient.
//
// Why it exists.  q(x) = fl(x / den) is monotone: x <= y implies x / den <= y / den exactly (den > 0), and rounding to nearest is
// monotone, so q(x) <= q(y); that holds over the whole ordered line -inf < ... < -0 <= +0 < ... < +inf (q(-inf) = -inf, q(+inf) = +inf,
// and q(-0) = -0 compares equal to q(+0)).  The floats with q(x) >= t therefore form an up-set of that line, X is its smallest member,
// and q(x) >= t <=> x >= X, q(x) < t <=> x < X for every non-NaN x.  For t not NaN the up-set is never empty: q(+inf) = +inf >= t.
//
// How it is found.  By bisection over the 2^32 - 2^24 floats of the ordered line (the usual sign-magnitude -> ordered-integer key), 32
// probes, each ONE float division of the host: the predicate that is bisected is the kernel's own test, not a model of it.  The host
// division is IEEE (x86-64 SSE / AArch64, no fast-math: FLT_EVAL_METHOD == 0 is asserted below), the device's is the correctly rounded
// one the library is built with (-fhip-fp32-correctly-rounded-divide-sqrt, subnormals kept): the same function of (x, den).
//
// Special thresholds:
//   t NaN        q(x) < NaN is false for every x           -> X = NaN   (x < NaN is false for every x)
//   t = +inf     q(x) < inf is true for every x < +inf     -> X = +inf  (found by the search: only q(+inf) reaches +inf)
//   t = -inf     never true                                -> X = -inf  (found by the search)
//   t = +-0      true for the x whose quotient is negative and does not round to -0: X is the smallest (negative, subnormal) float whose
//                quotient rounds to -0; t < 0 and subnormal t likewise need no special case
//   t so large that t * den overflows: X = +inf, as for t = +inf (every finite quotient is below t).
// den must be positive and finite (the only callers pass 2 * win * win); for any other den the function returns NaN: the test then
// fails no point, and the caller has to keep the division.
#if defined(FLT_EVAL_METHOD)
static_assert(FLT_EVAL_METHOD == 0, "float division must round to float");
#endif

static inline uint32_t av_lk_float_key(float x)          // order-preserving: key(a) < key(b) <=> a < b (with -0 < +0), NaNs excluded
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static inline float av_lk_key_float(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    memcpy(&x, &b, 4);
    return x;
}

static inline float av_lk_quotient_bound(float t, float den)
{
    if (t != t || !(den > 0.f) || den == INFINITY) return NAN;
    uint32_t lo = av_lk_float_key(-INFINITY), hi = av_lk_float_key(INFINITY);      // invariant: q(hi) >= t; every key below lo fails
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        volatile float q = av_lk_key_float(mid) / den;                            // volatile: the division is done, in float, as written
        if (q >= t) hi = mid; else lo = mid + 1;
    }
    return av_lk_key_float(hi);
}
