// noise_common.h — the device side of the portable seeded noise generator "philox4x32-10/v1", shared by noise.hip (the tensor
// fills) and the stochastic sampler steps (step_noise.h: the noise term of dpm.hip's and codenoise.hip's eta / SDE steps): the
// Philox4x32-10 block, the file's own ln, sin and cos, Box-Muller and the output rounding.  noise.hip's header states the
// expression; tests/noise_ref.py is its definition.  Every + - * / sqrt is one IEEE fp64 operation rounded on its own: every file
// that includes this header is built with -ffp-contract=off (csrc/Makefile).
#pragma once
#include <cmath>
#include <cstdint>

#include "vdx_common.h"

#define NOISE_HD __host__ __device__ __forceinline__

// seed and stream, low and high words: the block's key and the upper half of its counter
struct philox_key {
    uint32_t k0, k1, s0, s1;
};

NOISE_HD void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
}

NOISE_HD void philox4x32_10(uint64_t q, const philox_key& a, uint32_t (&c)[4]) {
    c[0] = (uint32_t)q;
    c[1] = (uint32_t)(q >> 32);
    c[2] = a.s0;
    c[3] = a.s1;
    uint32_t k0 = a.k0, k1 = a.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

NOISE_HD double noise_bits_to_double(uint64_t b) {
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
NOISE_HD uint64_t noise_double_to_bits(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

// ln u, u in (0, 1) a normal fp64
NOISE_HD double noise_ln(double u) {
    const uint64_t b = noise_double_to_bits(u);
    long long e = (long long)(b >> 52) - 1022;
    double m = noise_bits_to_double((b & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull);
    if (m < 0x1.6a09e667f3bcdp-1) {
        m = m * 2.0;
        e -= 1;
    }
    const double t = (m - 1.0) / (m + 1.0);
    const double z = t * t;
    double p = 0x1.642c8590b2164p-5;                                     // 1/23
    p = p * z + 0x1.8618618618618p-5;
    p = p * z + 0x1.af286bca1af28p-5;
    p = p * z + 0x1.e1e1e1e1e1e1ep-5;
    p = p * z + 0x1.1111111111111p-4;
    p = p * z + 0x1.3b13b13b13b14p-4;
    p = p * z + 0x1.745d1745d1746p-4;
    p = p * z + 0x1.c71c71c71c71cp-4;
    p = p * z + 0x1.2492492492492p-3;
    p = p * z + 0x1.999999999999ap-3;
    p = p * z + 0x1.5555555555555p-2;                                    // 1/3
    const double t2 = t * 2.0;
    const double lnm = t2 + t2 * (z * p);
    return (double)e * 0x1.62e42fefa39efp-1 + lnm;
}

// (cos, sin) of the angle (x + 0.5) 2^-32 of a turn
NOISE_HD void noise_cos_sin(uint32_t x, double& co, double& si) {
    const uint32_t o = x >> 29;
    uint32_t j = x & 0x1FFFFFFFu;
    if (o & 1u) j = 0x1FFFFFFFu - j;
    const double theta = (((double)j + 0.5) * 0x1p-29) * 0x1.921fb54442d18p-1;
    const double z = theta * theta;
    double ps = 0x1.952c77030ad4ap-49;                                   // 1/17!
    ps = ps * z + -0x1.ae7f3e733b81fp-41;
    ps = ps * z + 0x1.6124613a86d09p-33;
    ps = ps * z + -0x1.ae64567f544e4p-26;
    ps = ps * z + 0x1.71de3a556c734p-19;
    ps = ps * z + -0x1.a01a01a01a01ap-13;
    ps = ps * z + 0x1.1111111111111p-7;
    ps = ps * z + -0x1.5555555555555p-3;                                 // -1/3!
    const double s = theta + (theta * z) * ps;
    double pc = -0x1.6827863b97d97p-53;                                  // -1/18!
    pc = pc * z + 0x1.ae7f3e733b81fp-45;
    pc = pc * z + -0x1.93974a8c07c9dp-37;
    pc = pc * z + 0x1.1eed8eff8d898p-29;
    pc = pc * z + -0x1.27e4fb7789f5cp-22;
    pc = pc * z + 0x1.a01a01a01a01ap-16;
    pc = pc * z + -0x1.6c16c16c16c17p-10;
    pc = pc * z + 0x1.5555555555555p-5;
    pc = pc * z + -0x1.0000000000000p-1;                                 // -1/2!
    const double c = 1.0 + z * pc;
    const bool swap = ((o + 1u) >> 1) & 1u;
    co = swap ? s : c;
    si = swap ? c : s;
    if (((o + 2u) >> 2) & 1u) co = -co;
    if (o >= 4u) si = -si;
}

NOISE_HD void noise_box_muller(uint32_t xa, uint32_t xb, double& n0, double& n1) {
    const double u = ((double)xa + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * noise_ln(u));
    double co, si;
    noise_cos_sin(xb, co, si);
    n0 = r * co;
    n1 = r * si;
}

template <class T>
NOISE_HD T noise_out(double n, float sigma);
template <>
NOISE_HD float noise_out<float>(double n, float) { return (float)n; }
template <>
NOISE_HD f16 noise_out<f16>(double n, float sigma) { return (f16)((float)(f16)n * sigma); }
