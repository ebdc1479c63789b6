// rt_shared_math.h — fixed scalar algorithms that BOTH sides of the boundary run: the render kernel (hipcc, device) and the
// host library (g++, rust-tracing_amd/host/).  Built only from + - * / comparisons and bit moves, compiled without FMA
// contraction on either side, so device and host results agree bit for bit (include/rt_amd.h "Normative definitions").
//   rt_log   natural logarithm (ConstantMedium's free path, src/constant_medium.rs:48; and gamma below)
//   rt_exp   exponential (gamma below)
//   rt_gamma_encode   x^(1/2.2), the output stage's linear_to_gamma (src/color.rs:3-6)
//   rt_quantise       (256 * clamp(g, 0, 0.999)) as u8 (src/color.rs:12-19)
//   rt_tonemap, rt_luminance, rt_log_luminance_term, rt_log_average_result   the tone-mapping stage's operator and auto-exposure's terms
//   rt_rgbe_pack, rt_f32_of, rt_quantise16   the film formats' encoders: shared-exponent RGBE, f32 bits and the 16-bit gamma quantiser
//   rt_bloom_bright, rt_bloom_taps, rt_bloom_output   bloom's bright pass, one five-tap accumulation and its output value
//   rt_adaptive_converged   adaptive sampling's per-pixel stopping rule
// Coefficients: FreeBSD msun e_log.c / e_exp.c (public constants of the published algorithms).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace rtm {

RT_HD uint64_t f2u(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
RT_HD double u2f(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }

// x = 2^k * m, m in [sqrt(1/2), sqrt(2)); s = f / (2 + f), f = m - 1; degree-7 even/odd split polynomial; <= 1 ulp
RT_HD double rt_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t b = f2u(x);
    if ((b << 1) == 0) return -__builtin_inf();
    if (b >> 63) return __builtin_nan("");
    if ((b >> 52) == 0x7ff) return x;
    int64_t e = (int64_t)(b >> 52);
    if (e == 0) {
        x *= 18014398509481984.0;
        b = f2u(x);
        e = (int64_t)(b >> 52) - 54;
    }
    uint64_t mant = b & 0x000fffffffffffffull;
    int64_t k;
    double m;
    if (mant >= 0x6a09e667f3bcdull) { m = u2f(mant | 0x3fe0000000000000ull); k = e - 1022; }
    else                            { m = u2f(mant | 0x3ff0000000000000ull); k = e - 1023; }
    double f = m - 1.0;
    double s = f / (2.0 + f);
    double z = s * s;
    double w = z * z;
    double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    double R = t2 + t1;
    double hfsq = 0.5 * f * f;
    double dk = (double)k;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

// exp(x) for |x| <= 700 (beyond: +inf / 0; NaN stays NaN): k = round(x / ln2), r = x - k ln2 in two pieces, degree-5 Remez
// polynomial in r^2 for r (e^r + 1) / (e^r - 1), scaled by 2^k through the exponent field; <= 1 ulp
RT_HD double rt_exp(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, inv_ln2 = 1.44269504088896338700e+00,
                 P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    if (x != x) return x;
    if (x > 700.0) return __builtin_inf();
    if (x < -700.0) return 0.0;
    const double ax = x < 0.0 ? -x : x;
    double hi = x, lo = 0.0;
    int64_t k = 0;
    if (ax > 0.34657359027997264) { // 0.5 ln2
        const double t = (double)(int64_t)(inv_ln2 * x + (x < 0.0 ? -0.5 : 0.5));
        k = (int64_t)t;
        hi = x - t * ln2_hi;
        lo = t * ln2_lo;
        x = hi - lo;
    } else if (ax < 3.725290298461914e-09) { // 2^-28
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    return u2f(f2u(y) + ((uint64_t)k << 52)); // y in [0.5, 2], |k| <= 1010: the exponent field neither over- nor underflows
}

// linear_to_gamma: x.powf(1.0 / 2.2) (src/color.rs:3-6) as exp(ln(x) * (1 / 2.2)); powf's special cases for this exponent:
// +-0 -> 0, x < 0 -> NaN, +inf -> +inf, NaN -> NaN.  Relative error <= 2^-52 (1 + |ln x| / 2.2) of the exact power.
RT_HD double rt_gamma_encode(double x) {
    if (x != x) return x;
    if (x == 0.0) return 0.0;
    if (x < 0.0) return __builtin_nan("");
    if (x == __builtin_inf()) return x;
    return rt_exp(rt_log(x) * (1.0 / 2.2));
}

// `(256.0 * intensity.clamp(g)) as u8` with intensity = [0, 0.999] (src/color.rs:12-19): f64::clamp keeps NaN, and Rust's
// `NaN as u8` is 0
RT_HD uint8_t rt_quantise(double g) {
    if (g != g) return 0;
    const double c = g < 0.0 ? 0.0 : (g > 0.999 ? 0.999 : g);
    return (uint8_t)(256.0 * c);
}

// The tone-mapping operator of include/rt_amd.h "tone mapping", per channel, on the exposed value x; w2 = white * white (Reinhard only).
// Applied where 0 < x < +inf; zero, a negative, NaN and +-inf pass through to rt_gamma_encode / rt_quantise unchanged.  Every
// operation is rounded on its own, in the header's order.  op: RT_TONEMAP_CLAMP 0, RT_TONEMAP_REINHARD 1, RT_TONEMAP_ACES 2.
RT_HD double rt_tonemap(int32_t op, double x, double w2) {
    if (!(x > 0.0) || x == __builtin_inf()) return x;
    if (op == 1) { // Reinhard's extended operator; w2 = +inf: r is exactly 1 and y = x / (1 + x)
        double r = x / w2;
        r = 1.0 + r;
        const double num = x * r;
        const double den = 1.0 + x;
        return num / den;
    }
    if (op == 2) { // Narkowicz's fit of the ACES filmic curve
        double a = 2.51 * x;
        a = a + 0.03;
        const double num = x * a;
        double b = 2.43 * x;
        b = b + 0.59;
        double den = x * b;
        den = den + 0.14;
        return num / den;
    }
    return x;
}

// The film formats' encoders (include/rt_amd.h "film output"), on the tone-mapped value y.  Bit moves and exact multiplications by powers
// of two only: no rounding mode, denormal mode or library call that could differ between the two sides.
// RT_FILM_RGBE: Radiance's shared exponent, R in the low byte and the exponent byte on top.  c = y where y > 0 (+inf included), else 0;
// c = min(c, 255 * 2^119); v = the largest c; v < 2^-128: the zero pixel.  Else e with 2^(e-1) <= v < 2^e from v's exponent field (v is
// normal), b_k = (u8)(c_k * 2^(8-e)) — exact, then truncated — and E = e + 128 in 1..255.
RT_HD uint32_t rt_rgbe_pack(double yr, double yg, double yb) {
    const double top = 255.0 * u2f((uint64_t)(119 + 1023) << 52);
    double c[3] = {yr > 0.0 ? yr : 0.0, yg > 0.0 ? yg : 0.0, yb > 0.0 ? yb : 0.0};
    for (int k = 0; k < 3; ++k) c[k] = c[k] > top ? top : c[k];
    double v = c[0];
    if (c[1] > v) v = c[1];
    if (c[2] > v) v = c[2];
    if (v < u2f((uint64_t)(1023 - 128) << 52)) return 0u;
    const int32_t e = (int32_t)((f2u(v) >> 52) & 0x7ff) - 1022; // -127 .. 127
    const double s = u2f((uint64_t)(8 - e + 1023) << 52);       // 2^(8-e), a normal number
    return (uint32_t)(uint8_t)(c[0] * s) | ((uint32_t)(uint8_t)(c[1] * s) << 8) | ((uint32_t)(uint8_t)(c[2] * s) << 16) | ((uint32_t)(e + 128) << 24);
}

// RT_FILM_F32: the bits of (float)y rounded to nearest, ties to even: overflow gives +-inf, signs are kept (-0.0 too), what lies below
// f32's normal range becomes an f32 subnormal or +-0, and every NaN becomes 0x7fc00000.
RT_HD uint32_t rt_f32_of(double y) {
    const uint64_t b = f2u(y);
    const uint32_t sign = (uint32_t)(b >> 63) << 31, ef = (uint32_t)(b >> 52) & 0x7ffu;
    const uint64_t man = b & 0x000fffffffffffffull;
    if (ef == 0x7ffu) return man ? 0x7fc00000u : sign | 0x7f800000u;
    const int32_t e = (int32_t)ef - 1023 + 127; // the f32 exponent field of a normal result
    if (e >= 255) return sign | 0x7f800000u;
    if (ef == 0 || e < -30) return sign;        // (below 2^-157: far under half of f32's smallest subnormal, 2^-150)
    const int shift = e >= 1 ? 29 : 29 + (1 - e); // 52 - 23 bits go; a subnormal result loses 1 - e more
    const uint64_t sig = man | (1ull << 52), half = 1ull << (shift - 1), rem = sig & ((half << 1) - 1u);
    uint64_t q = sig >> shift;
    if (rem > half || (rem == half && (q & 1u))) ++q;
    // a normal q holds the implicit bit, which counts as one step of the exponent field; a carry out of the mantissa is the next step
    // (up to the field of +inf), and a subnormal that rounds up to 2^23 is the smallest normal
    return sign | (((uint32_t)(e >= 1 ? e - 1 : 0) << 23) + (uint32_t)q);
}

// RT_FILM_RGB16: (u16)(65536 * clamp(g, 0, 0.99999)), NaN -> 0.  Its high byte is rt_quantise(g): both scalings are exact and both
// clamps land in 255.
RT_HD uint16_t rt_quantise16(double g) {
    if (g != g) return 0;
    const double c = g < 0.0 ? 0.0 : (g > 0.99999 ? 0.99999 : g);
    return (uint16_t)(65536.0 * c);
}

// Rec. 709 luminance of a linear colour, in this order: ((0.2126 r + 0.7152 g) + 0.0722 b)
RT_HD double rt_luminance(double r, double g, double b) { return ((0.2126 * r) + (0.7152 * g)) + (0.0722 * b); }

// Auto-exposure's per-pixel term (include/rt_amd.h "tone mapping"): the pixel counts iff its three means are finite and its
// luminance is >= 0; a counting pixel contributes rt_log(delta + L), any other +0.0 and count 0.
RT_HD double rt_log_luminance_term(double mr, double mg, double mb, double delta, uint32_t *counts) {
    *counts = 0;
    if (((f2u(mr) >> 52) & 0x7ff) == 0x7ff || ((f2u(mg) >> 52) & 0x7ff) == 0x7ff || ((f2u(mb) >> 52) & 0x7ff) == 0x7ff) return 0.0;
    const double L = rt_luminance(mr, mg, mb);
    if (!(L >= 0.0)) return 0.0;
    *counts = 1;
    return rt_log(delta + L);
}

// What the reduction's last level makes of the total T and the count (include/rt_amd.h "tone mapping", Result): out4 = log_mean, Lavg,
// (double)count, scale.  auto_key == 0 (rt_log_average_luminance_device) writes 0 in scale's place.
RT_HD void rt_log_average_result(double T, uint32_t count, double exposure, double auto_key, double out4[4]) {
    double log_mean = 0.0, lavg = 0.0, scale = exposure;
    if (count != 0) {
        log_mean = T / (double)count;
        lavg = rt_exp(log_mean);
        scale = exposure * (auto_key / lavg);
    }
    out4[0] = log_mean;
    out4[1] = lavg;
    out4[2] = (double)count;
    out4[3] = auto_key > 0.0 ? scale : 0.0;
}

// Bloom (include/rt_amd.h "bloom"), every operation rounded on its own, in the header's order.
// The bright pass of one pixel with means (mr, mg, mb): it is a source iff the three means and its luminance L are finite and
// L > threshold; a source's b0 is its means times k = (L - threshold) / L, any other pixel's +0.0.
RT_HD void rt_bloom_bright(double mr, double mg, double mb, double threshold, double b0[3]) {
    b0[0] = b0[1] = b0[2] = 0.0;
    if (((f2u(mr) >> 52) & 0x7ff) == 0x7ff || ((f2u(mg) >> 52) & 0x7ff) == 0x7ff || ((f2u(mb) >> 52) & 0x7ff) == 0x7ff) return;
    const double L = rt_luminance(mr, mg, mb);
    if (((f2u(L) >> 52) & 0x7ff) == 0x7ff || !(L > threshold)) return;
    const double d = L - threshold;
    const double k = d / L;
    b0[0] = mr * k;
    b0[1] = mg * k;
    b0[2] = mb * k;
}

// One five-tap accumulation: acc = +0.0; for d = -2 .. 2 in order, acc = acc + (h[d] * v[d + 2]) for the taps whose bit d + 2 of
// `inside` is set (the others lie outside the frame and are skipped; their v is not read).  h = (1/16, 1/4, 3/8, 1/4, 1/16).
RT_HD double rt_bloom_taps(const double v[5], uint32_t inside) {
    double acc = 0.0;
    if (inside & 1u) acc = acc + (0.0625 * v[0]);
    if (inside & 2u) acc = acc + (0.25 * v[1]);
    if (inside & 4u) acc = acc + (0.375 * v[2]);
    if (inside & 8u) acc = acc + (0.25 * v[3]);
    if (inside & 16u) acc = acc + (0.0625 * v[4]);
    return acc;
}

// The output value: g = A_K / (double)K; out = m + (strength * g)
RT_HD double rt_bloom_output(double m, double a, int32_t levels, double strength) {
    const double g = a / (double)levels;
    const double t = strength * g;
    return m + t;
}

// Adaptive sampling's convergence rule (include/rt_amd.h rt_render_adaptive), for a pixel with n >= 2 samples, channel sums S
// and sums of squares Q; f64 in exactly this order, no FMA:
//   m_c = S_c / n,  v_c = (Q_c - S_c * m_c) / (n - 1),  e2 = max(v_r, v_g, v_b) / n,  L = ((m_r + m_g) + m_b) / 3,
//   tol = rel * L + abs,  converged <=> e2 <= tol * tol.   A non-finite S or Q (or a NaN variance) never converges.
RT_HD bool rt_adaptive_converged(const double S[3], const double Q[3], int32_t n, double rel_threshold, double abs_threshold) {
    for (int c = 0; c < 3; ++c)
        if (((f2u(S[c]) >> 52) & 0x7ff) == 0x7ff || ((f2u(Q[c]) >> 52) & 0x7ff) == 0x7ff) return false;
    const double dn = (double)n;
    double m[3], v[3];
    for (int c = 0; c < 3; ++c) {
        m[c] = S[c] / dn;
        v[c] = (Q[c] - S[c] * m[c]) / (dn - 1.0);
        if (v[c] != v[c]) return false;
    }
    double vmax = v[0];
    if (v[1] > vmax) vmax = v[1];
    if (v[2] > vmax) vmax = v[2];
    const double e2 = vmax / dn;
    const double L = ((m[0] + m[1]) + m[2]) / 3.0;
    const double tol = rel_threshold * L + abs_threshold;
    return e2 <= tol * tol;
}

} // namespace rtm
