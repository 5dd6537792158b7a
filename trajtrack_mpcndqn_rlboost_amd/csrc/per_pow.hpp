// libm_pow(x, y): the C library's float64 pow restated operation by operation, so that a priority computed on the device
// equals math.pow of the numpy twin (and with it the reference's own leaves) BIT FOR BIT.  The device library's pow is within
// an ulp but rounds about one argument in seven differently, and a leaf that is one ulp off moves every sum above it.
//
// What is restated is the library's build for processors with fused multiply-add -- the one a host of this project runs
// (every x86-64 with AVX2, every aarch64): each fma() below is a fused operation there, each other operation a rounded one,
// read off that build's instruction stream; the file is compiled with -ffp-contract=off so that nothing else is fused.
// Covered: x positive and normal, y normal with 2^-65 <= |y| < 2^63, |y log x| < 512 -- everything a priority can be.
// Outside of that (zero, subnormal, infinite, NaN, overflow, underflow) the caller's fallback is the device library's pow, whose
// special values are the standard's.
#pragma once
#include <cmath>
#include <cstdint>

#include "per_pow_tables.hpp"

namespace pergpu {

PER_POW_FN inline uint64_t as_bits(double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u; }
PER_POW_FN inline double as_double(uint64_t u) { double v; __builtin_memcpy(&v, &u, 8); return v; }

// returns false when (x, y) is outside the covered range
PER_POW_FN inline bool libm_pow(double x, double y, double* out) {
    const uint64_t ix = as_bits(x), iy = as_bits(y);
    const uint32_t topx = (uint32_t)(ix >> 52), topy = (uint32_t)(iy >> 52) & 0x7ff;
    if (topx - 1u > 0x7fdu || topy - 0x3beu > 0x7fu) return false;
    // log(x) = hi + lo
    const uint64_t tmp = ix - 0x3fe6955500000000ull;
    const int i = (int)((tmp >> 45) & 127);
    const double kd = (double)(int32_t)((int64_t)tmp >> 52);
    const double z = as_double(ix - (tmp & 0xfff0000000000000ull));
    const double invc = POW_LOG_TAB[i][0], logc = POW_LOG_TAB[i][1], logctail = POW_LOG_TAB[i][2];
    const double t1 = fma(kd, POW_LN2HI, logc);
    const double r = fma(z, invc, -1.0);
    const double ar = r * POW_A0;
    const double lo1 = fma(kd, POW_LN2LO, logctail);
    const double q12 = fma(r, POW_A2, POW_A1);
    const double q34 = fma(r, POW_A4, POW_A3);
    const double t2 = r + t1;
    const double ar2 = r * ar;
    const double d12 = t1 - t2;
    const double ar3 = r * ar2;
    const double lo3 = fma(ar, r, -ar2);
    const double lo2 = d12 + r;
    const double q56 = fma(r, POW_A6, POW_A5);
    const double hi = t2 + ar2;
    const double d2h = t2 - hi;
    const double q36 = fma(q56, ar2, q34);
    const double lo4 = d2h + ar2;
    const double p = fma(ar2, q36, q12);
    double lo = lo1 + lo2;
    lo = lo + lo3;
    lo = lo + lo4;
    lo = fma(ar3, p, lo);
    const double lhi = hi + lo;
    double ltail = hi - lhi;
    ltail = ltail + lo;
    // y log(x) = ehi + elo
    const double ehi = y * lhi;
    const double elo = fma(y, ltail, fma(lhi, y, -ehi));
    // exp(ehi + elo)
    const uint32_t abstop = (uint32_t)(as_bits(ehi) >> 52) & 0x7ff;
    if (abstop - 0x3c9u > 0x3eu) {
        if (abstop < 0x3c9u) { *out = 1.0 + ehi; return true; }      // |y log x| < 2^-54
        return false;
    }
    const double ks = fma(ehi, EXP_INVLN2N, EXP_SHIFT);
    const uint64_t ki = as_bits(ks);
    const double k = ks - EXP_SHIFT;
    double rr = fma(k, EXP_NEGLN2HIN, ehi);
    rr = fma(k, EXP_NEGLN2LON, rr);
    const int idx = 2 * (int)(ki & 127);
    const uint64_t sbits = EXP_TAB[idx + 1] + (ki << 45);
    rr = elo + rr;
    const double a = fma(rr, EXP_C3, EXP_C2);
    const double b = rr + as_double(EXP_TAB[idx]);
    const double r2 = rr * rr;
    const double c = fma(rr, EXP_C5, EXP_C4);
    const double d = fma(a, r2, b);
    const double r4 = r2 * r2;
    const double e = fma(c, r4, d);
    const double scale = as_double(sbits);
    *out = fma(e, scale, scale);
    return true;
}

}  // namespace pergpu
