// lk_bound_harness.cpp -- av_lk_quotient_bound of uav_airvision_amd/csrc/lk_host.h (the bound the 16-lane LK kernel compares its
// eigenvalue numerator with, in place of dividing it by 2 win^2) on the CPU, no HIP (tests/test_lk_bound.py builds and runs this).
// For every threshold t given on the command line as the hexadecimal bits of a float, and den = 450:
//   * computes X = av_lk_quotient_bound(t, den);
//   * walks every float within 64 ulps of X (along the ordered line -inf .. +inf, clipped at its ends) and the two infinities, and counts
//     the x for which  fl(x / den) < t  differs from  x < X  (the division is the host's own float division);
//   * prints "<t bits> <X bits> <floats checked> <mismatches>", so that the caller can repeat the check with its own arithmetic.
#include <stdio.h>
#include <stdlib.h>

#include "lk_host.h"

static uint32_t bits_of(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
static float float_of(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

int main(int argc, char** argv)
{
    const float den = 450.f;
    for (int i = 1; i < argc; ++i) {
        const float t = float_of((uint32_t)strtoul(argv[i], nullptr, 16));
        const float X = av_lk_quotient_bound(t, den);
        long checked = 0, bad = 0;
        auto probe = [&](float x) {
            volatile float q = x / den;
            ++checked;
            if ((q < t) != (x < X)) ++bad;
        };
        probe(-INFINITY);
        probe(INFINITY);
        probe(NAN);
        if (X == X) {
            const uint32_t lo = av_lk_float_key(-INFINITY), hi = av_lk_float_key(INFINITY), kx = av_lk_float_key(X);
            const uint32_t a = kx - lo > 64 ? kx - 64 : lo, b = hi - kx > 64 ? kx + 64 : hi;
            for (uint32_t k = a;; ++k) { probe(av_lk_key_float(k)); if (k == b) break; }
        } else {
            // no bound: the test must fail nothing, whatever x (a sample of the line: every 2^16-th float)
            for (uint64_t k = av_lk_float_key(-INFINITY); k <= av_lk_float_key(INFINITY); k += 65536) probe(av_lk_key_float((uint32_t)k));
        }
        printf("%08x %08x %ld %ld\n", bits_of(t), bits_of(X), checked, bad);
    }
    return 0;
}
