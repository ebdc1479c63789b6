// rt_reject.hpp — the accept / reject decision of the two rejection samplers, settled in f32 (rt_device_scene.h random_in_unit_sphere,
// src/vec3.rs:54-61; rt_kernel.hip Camera::get_ray's random_in_unit_disk, src/vec3.rs:77-88).  Host and device compile the same code.
// A pass of either loop draws a candidate with gen_range(-1.0..1.0) per coordinate and keeps it iff its squared length, in f64 and in
// the reference's operation order, is below 1.  All the f64 arithmetic of a pass produces is that one bit; the classifier below
// produces it from the raw draws in f32 and says "uncertain" where it cannot, and only an uncertain candidate evaluates the exact
// predicate.  The classifier can only err towards "uncertain" (tests/test_gpu_reject_sampler.py, tests/test_reject_sampler_host.py).
//
// Exact coordinates.  Rng::range(-1, 1) of a draw w takes m = w >> 12 (52 bits) and computes
//     v = 1 + m 2^-52 (bit pattern)      a = v - 1 = m 2^-52      b = a * 2 = m 2^-51      x = b + -1 = m 2^-51 - 1
// and every one of the three operations is exact: a and b are m scaled by a power of two, and x is a multiple of 2^-51 of magnitude
// at most 1, 52 significant bits.  So x = m 2^-51 - 1 in [-1, 1), whatever order or contraction the operations are compiled with
// (reject_coord below is range's arithmetic; the render kernel builds the kept candidate's coordinates with it once, after the loop).
//
// f32 approximation.  From the draw's high word h = w >> 32:   H = (float)h  (one conversion, round to nearest: the top 24 significant
// bits of the draw),   x~ = fma(H, 2^-31, -1)  (one fma).  Per coordinate
//     m 2^-51 - h 2^-31 = (bits 12..31 of w) 2^-51  in [0, 2^-31)                     (the low bits the high word leaves out)
//     |H - h| <= 2^7    (h < 2^32: half an ulp of [2^31, 2^32)),  2^-24 in x
//     the fma's rounding: H 2^-31 - 1 is in [-1, 1]; at most half an ulp of [1/2, 1) = 2^-25
// together  |x - x~| <= 2^-31 + 2^-24 + 2^-25 < 2^-23,  and with |x|, |x~| <= 1:   |x^2 - x~^2| = |x - x~| |x + x~| < 2^-22.
// The squared length  l~ = fma(z~, z~, fma(y~, y~, x~ * x~))  (explicit fmas: this filter is not part of the f64 arithmetic
// contract) rounds three times, at results of at most 1, 2 and 3:  2^-25 + 2^-24 + 2^-23 = 7 * 2^-25.
// The f64 len2 = x*x + y*y + z*z itself is off the real sum of squares by its own five roundings: three products of at most 1
// (2^-54 each), sums of at most 2 and 4 (2^-53, 2^-52): under 2^-51.
//     sphere:  |l~ - len2_f64| < 3 * 2^-22 + 7 * 2^-25 + 2^-51 = 31 * 2^-25 + 2^-51 < 2^-20                     =: REJECT_EB_SPHERE
//     disk  :  dx*dx + dy*dy + 0.0*0.0 (the last term and its addition are exact):
//              2 * 2^-22 + (2^-25 + 2^-24) + (2 * 2^-54 + 2^-53) = 19 * 2^-25 + 2^-52 < 20 * 2^-25 = 1.25 * 2^-21 =: REJECT_EB_DISK
// The band is the power of two that is at least twice the larger bound: 2^-19 for both (2 * 1.25 * 2^-21 exceeds 2^-20).  1 - 2^-19
// and 1 + 2^-19 are floats, so the two comparisons are exact:
//     l~ < 1 - band  =>  len2_f64 < 1 - 2^-19 + 2^-20 < 1   certain accept        l~ > 1 + band  =>  len2_f64 > 1   certain reject
// and anything else is uncertain: a shell of 4 pi band / 8 (the cube's volume is 8) — about 3e-6 of the candidates.
#pragma once
#include "rt_shared_math.h"

namespace rtm {

constexpr float REJECT_EB_SPHERE = 0x1p-20f;  // bound on |l~ - len2_f64|, three coordinates
constexpr float REJECT_EB_DISK = 0x1.4p-21f;  // ... two coordinates
constexpr float REJECT_BAND = 0x1p-19f;       // >= 2 * the larger of the two
static_assert(REJECT_BAND >= 2.0f * REJECT_EB_SPHERE && REJECT_BAND >= 2.0f * REJECT_EB_DISK, "the band covers both bounds twice");

enum : int { REJECT_NO = 0, REJECT_YES = 1, REJECT_UNCERTAIN = 2 };

// gen_range(-1.0..1.0) of a raw draw: Rng::range's three operations (rt_device_math.h; exact, see above)
RT_HD double reject_coord(uint64_t draw) {
    const double value1_2 = u2f((draw >> 12) | 0x3ff0000000000000ull);
    return (value1_2 - 1.0) * (1.0 - -1.0) + -1.0;
}
RT_HD float reject_coord32(uint64_t draw) {
    const uint32_t h = (uint32_t)(draw >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    // (spelled out: the compiler widens the conversion of a shifted 64-bit value back to a 64-bit one, five instructions for this one)
    float H;
    asm("v_cvt_f32_u32 %0, %1" : "=v"(H) : "v"(h));
#else
    const float H = (float)h;
#endif
    return __builtin_fmaf(H, 0x1p-31f, -1.0f);
}
RT_HD int reject_classify(float l) { return l < 1.0f - REJECT_BAND ? REJECT_YES : (l > 1.0f + REJECT_BAND ? REJECT_NO : REJECT_UNCERTAIN); }

// unit sphere: the f32 verdict, and the reference's predicate (len2 in Vec3::dot's order, src/vec3.rs:104-106)
RT_HD int reject_sphere_f32(uint64_t wx, uint64_t wy, uint64_t wz) {
    const float x = reject_coord32(wx), y = reject_coord32(wy), z = reject_coord32(wz);
    return reject_classify(__builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
}
RT_HD bool reject_sphere_exact(uint64_t wx, uint64_t wy, uint64_t wz) {
    const double x = reject_coord(wx), y = reject_coord(wy), z = reject_coord(wz);
    const double xx = x * x, yy = y * y, zz = z * z; // (no contraction: -ffp-contract=off wherever this header is compiled)
    const double s = xx + yy;
    return s + zz < 1.0;
}
// unit disk: Vec3::new(x, y, 0.0).length_squared() < 1.0
RT_HD int reject_disk_f32(uint64_t wx, uint64_t wy) {
    const float x = reject_coord32(wx), y = reject_coord32(wy);
    return reject_classify(__builtin_fmaf(y, y, x * x));
}
RT_HD bool reject_disk_exact(uint64_t wx, uint64_t wy) {
    const double x = reject_coord(wx), y = reject_coord(wy);
    const double xx = x * x, yy = y * y, zz = 0.0 * 0.0;
    const double s = xx + yy;
    return s + zz < 1.0;
}

} // namespace rtm
