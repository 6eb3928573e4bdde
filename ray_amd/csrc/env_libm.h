// env_libm.h -- sinf, cosf, acosf and atan2f as the C library the reference is built against computes them, restated so that the device
// and the host produce the SAME BITS as that library (env_qtree.h needs them: a tap of the environment map's quadtree whose map
// coordinate is a whole number in exact arithmetic -- every tap of a map whose width is a power of two -- reads the texel the last bit
// of atan2f names, and the reference's quadtree is what frames are held against).  The algorithms are public: acosf, atanf and atan2f
// are fdlibm's float routines (e_acosf.c, s_atanf.c, e_atan2f.c: single-precision arithmetic in a fixed order), sinf and cosf the
// double-precision polynomials of the optimized-routines project (sincosf.h: one reduction by pi / 2, two polynomials).  IEEE
// operations in a STATED ORDER without contraction, like every shared header here; only the range the taps use is restated -- finite
// arguments, |x| < 120 for sinf / cosf -- and anything else goes to the platform's function.  tests/test_env_hostsim.py holds these
// against the C library's own functions bit for bit, on the taps' arguments and on random ones.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rt_base.h"

namespace rayhip_env_libm {

using rt::float_as_uint;
using rt::uint_as_float;

// ---- sinf / cosf ----------------------------------------------------------------------------------------------------------------
struct SinCosTable {
    double hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3;
};
RT_HD SinCosTable sincos_table(const bool negated) {
    const double f = negated ? -1.0 : 1.0; // (the second table: the cosine polynomial negated)
    return SinCosTable{0x1.45F306DC9C883p+23, 0x1.921FB54442D18p0, f * 0x1p0, f * -0x1.ffffffd0c621cp-2, f * 0x1.55553e1068f19p-5,
                       f * -0x1.6c087e89a359dp-10, f * 0x1.99343027bf8c3p-16, -0x1.555545995a603p-3, 0x1.1107605230bc4p-7, -0x1.994eb3774cf24p-13};
}
// the table's sign[4] = {1, -1, -1, 1}, as a select: no indexed table, which on the device would live in scratch memory
RT_HD double quadrant_sign(const int n) { return (((n >> 1) ^ n) & 1) != 0 ? -1.0 : 1.0; }
RT_HD uint32_t abstop12(const float x) { return (float_as_uint(x) >> 20) & 0x7ffu; }
RT_HD float sincos_poly(const double x, const double x2, const SinCosTable &p, const int n) {
    if ((n & 1) == 0) {
        const double x3 = x * x2;
        const double s1 = p.s2 + x2 * p.s3;
        const double x7 = x3 * x2;
        const double s = x + x3 * p.s1;
        return float(s + x7 * s1);
    }
    const double x4 = x2 * x2;
    const double c2 = p.c3 + x2 * p.c4;
    const double c1 = p.c0 + x2 * p.c1;
    const double x6 = x4 * x2;
    const double c = c1 + x4 * p.c2;
    return float(c + x6 * c2);
}
RT_HD double reduce_fast(const double x, const SinCosTable &p, int &n) {
    const double r = x * p.hpi_inv;
    n = (int32_t(r) + 0x800000) >> 24;
    return x - double(n) * p.hpi;
}
RT_HD float sin_f(const float y) {
    const double x = double(y);
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        if (abstop12(y) < abstop12(0x1p-12f)) {
            return y;
        }
        return sincos_poly(x, x * x, sincos_table(false), 0);
    }
    if (abstop12(y) < abstop12(120.0f)) {
        int n = 0;
        const SinCosTable p = sincos_table(false);
        const double r = reduce_fast(x, p, n);
        const double s = quadrant_sign(n);
        return sincos_poly(r * s, r * r, sincos_table((n & 2) != 0), n);
    }
    return sinf(y);
}
RT_HD float cos_f(const float y) {
    const double x = double(y);
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
        if (abstop12(y) < abstop12(0x1p-12f)) {
            return 1.0f;
        }
        return sincos_poly(x, x * x, sincos_table(false), 1);
    }
    if (abstop12(y) < abstop12(120.0f)) {
        int n = 0;
        const SinCosTable p = sincos_table(false);
        const double r = reduce_fast(x, p, n);
        const double s = quadrant_sign(n + 1);
        return sincos_poly(r * s, r * r, sincos_table(((n + 1) & 2) != 0), n ^ 1);
    }
    return cosf(y);
}

// ---- acosf (|x| <= 1) -------------------------------------------------------------------------------------------------------------
RT_HD float acos_ratio(const float z) {
    const float pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f, pS4 = 7.9153501429e-04f,
                pS5 = 3.4793309169e-05f, qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const float q = 1.0f + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    return p / q;
}
RT_HD float acos_f(const float x) {
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const uint32_t hx = float_as_uint(x), ix = hx & 0x7fffffffu;
    if (ix == 0x3f800000u) {
        return (hx >> 31) == 0 ? 0.0f : pi + 2.0f * pio2_lo;
    }
    if (ix > 0x3f800000u) {
        return acosf(x);
    }
    if (ix < 0x3f000000u) {
        if (ix <= 0x23000000u) {
            return pio2_hi + pio2_lo;
        }
        const float r = acos_ratio(x * x);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if ((hx >> 31) != 0) {
        const float z = (1.0f + x) * 0.5f;
        const float s = sqrtf(z);
        const float r = acos_ratio(z);
        const float w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    const float z = (1.0f - x) * 0.5f;
    const float s = sqrtf(z);
    const float df = uint_as_float(float_as_uint(s) & 0xfffff000u);
    const float c = (z - df * df) / (s + df);
    const float r = acos_ratio(z);
    const float w = r * s + c;
    return 2.0f * (df + w);
}

// ---- atanf, atan2f (finite arguments) ---------------------------------------------------------------------------------------------
RT_HD float atan_f(float x) {
    // atanhi[4] and atanlo[4], read through selects further down (an indexed table would live in scratch memory on the device)
    const float hi0 = 4.6364760399e-01f, hi1 = 7.8539812565e-01f, hi2 = 9.8279368877e-01f, hi3 = 1.5707962513e+00f;
    const float lo0 = 5.0121582440e-09f, lo1 = 3.7748947079e-08f, lo2 = 3.4473217170e-08f, lo3 = 7.5497894159e-08f;
    const float aT[11] = {3.3333334327e-01f,  -2.0000000298e-01f, 1.4285714924e-01f,  -1.1111110449e-01f, 9.0908870101e-02f, -7.6918758452e-02f,
                          6.6610731184e-02f, -5.8335702866e-02f, 4.9768779427e-02f, -3.6531571299e-02f, 1.6285819933e-02f};
    const uint32_t hx = float_as_uint(x), ix = hx & 0x7fffffffu;
    int id;
    if (ix >= 0x4c000000u) { // |x| >= 2^25
        if (ix > 0x7f800000u) {
            return x + x;
        }
        return (hx >> 31) == 0 ? hi3 + lo3 : -hi3 - lo3;
    }
    if (ix < 0x3ee00000u) { // |x| < 0.4375
        if (ix < 0x31000000u) {
            return x;
        }
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000u) {     // |x| < 1.1875
            if (ix < 0x3f300000u) { // 7/16 <= |x| < 11/16
                id = 0;
                x = (2.0f * x - 1.0f) / (2.0f + x);
            } else {
                id = 1;
                x = (x - 1.0f) / (x + 1.0f);
            }
        } else {
            if (ix < 0x401c0000u) { // |x| < 2.4375
                id = 2;
                x = (x - 1.5f) / (1.0f + 1.5f * x);
            } else {
                id = 3;
                x = -1.0f / x;
            }
        }
    }
    const float z = x * x;
    const float w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) {
        return x - x * (s1 + s2);
    }
    const float hi = id == 0 ? hi0 : id == 1 ? hi1 : id == 2 ? hi2 : hi3, lo = id == 0 ? lo0 : id == 1 ? lo1 : id == 2 ? lo2 : lo3;
    const float r = hi - ((x * (s1 + s2) - lo) - x);
    return (hx >> 31) != 0 ? -r : r;
}
RT_HD float atan2_f(const float y, const float x) {
    const float tiny = 1.0e-30f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const uint32_t hx = float_as_uint(x), hy = float_as_uint(y), ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix >= 0x7f800000u || iy >= 0x7f800000u) {
        return atan2f(y, x);
    }
    if (hx == 0x3f800000u) {
        return atan_f(y);
    }
    const uint32_t m = ((hy >> 31) & 1u) | ((hx >> 30) & 2u);
    if (iy == 0) {
        return m < 2 ? y : (m == 2 ? pi + tiny : -pi - tiny);
    }
    if (ix == 0) {
        return (hy >> 31) != 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    }
    const int k = (int(iy) - int(ix)) >> 23;
    float z;
    if (k > 60) {
        z = pi_o_2 + 0.5f * pi_lo;
    } else if ((hx >> 31) != 0 && k < -60) {
        z = 0.0f;
    } else {
        z = atan_f(fabsf(y / x));
    }
    switch (m) {
    case 0:
        return z;
    case 1:
        return uint_as_float(float_as_uint(z) ^ 0x80000000u);
    case 2:
        return pi - (z - pi_lo);
    default:
        return (z - pi_lo) - pi;
    }
}

} // namespace rayhip_env_libm
