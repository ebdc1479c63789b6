// rt_metrics_shared.h — frame metrics (include/rt_amd.h "frame metrics"): everything the level kernel (rt_metrics.hip) and the host
// mirror (rth_frame_error, rth_frame_noise in host/capi.cpp) share, so that both compile the same text and give the same bits.
//   rtm::rt_error_*, rtm::rt_noise_*   per call, the pixel term, the combine of two entries and the final values (RT_HD, f64, every
//                                      operation rounded on its own in the header's order; rt_log for the one logarithm)
//   rtmt::                             the host side of the two params-carrying calls: defaults, struct sizes, the checks in the
//                                      header's order with the messages' tails, and the workspace size.  Plain C++, no device code.
// An entry of the reduction tree is a small record: ACCS doubles and an integer count.  The neutral entry (a pixel that does not count,
// and the padding of a level) is all +0.0 with count 0.
#pragma once
#include "rt_amd.h"
#include "rt_shared_math.h"

#include <cmath>
#include <cstring>

namespace rtm {

RT_HD bool rt_metrics_finite(double x) { return ((f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
RT_HD double rt_metrics_max(double a, double b) { return a < b ? b : a; } // the header's rule for maxima
RT_HD double rt_metrics_abs(double x) { return u2f(f2u(x) & 0x7fffffffffffffffull); }

// ---- rt_frame_error_device: accumulators T_sq, T_rel, T_ab, T_d (sums) and max_abs (a maximum) ----
constexpr int RT_ERROR_ACCS = 5;

// One pixel with means m and reference means r.  It counts iff all six are finite; a counting pixel's entry is, per channel,
// d = m - r, sq = d * d, ab = |d|, den = (r * r) + eps, rel = sq / den, and per pixel (t_r + t_g) + t_b of sq, rel, ab and d and the
// maximum of ab.  Any other pixel is the neutral entry.
RT_HD void rt_error_term(const double m[3], const double r[3], double eps, double e[RT_ERROR_ACCS], uint32_t *count) {
    *count = 0;
    for (int k = 0; k < RT_ERROR_ACCS; ++k) e[k] = 0.0;
    for (int c = 0; c < 3; ++c)
        if (!rt_metrics_finite(m[c]) || !rt_metrics_finite(r[c])) return;
    double sq[3], rel[3], ab[3], d[3];
    for (int c = 0; c < 3; ++c) {
        d[c] = m[c] - r[c];
        sq[c] = d[c] * d[c];
        ab[c] = rt_metrics_abs(d[c]);
        const double den = (r[c] * r[c]) + eps;
        rel[c] = sq[c] / den;
    }
    e[0] = (sq[0] + sq[1]) + sq[2];
    e[1] = (rel[0] + rel[1]) + rel[2];
    e[2] = (ab[0] + ab[1]) + ab[2];
    e[3] = (d[0] + d[1]) + d[2];
    e[4] = rt_metrics_max(rt_metrics_max(ab[0], ab[1]), ab[2]);
    *count = 1;
}

// a = a (+) b
RT_HD void rt_error_combine(double a[RT_ERROR_ACCS], uint32_t *ca, const double b[RT_ERROR_ACCS], uint32_t cb) {
    a[0] = a[0] + b[0];
    a[1] = a[1] + b[1];
    a[2] = a[2] + b[2];
    a[3] = a[3] + b[3];
    a[4] = rt_metrics_max(a[4], b[4]);
    *ca = *ca + cb;
}

// out8 = count, mse, rmse, rel_mse, mae, bias, max_abs, psnr of the tree's last entry; all 0 where nothing counts
RT_HD void rt_error_result(const double e[RT_ERROR_ACCS], uint32_t count, double peak, double out8[8]) {
    for (int k = 0; k < 8; ++k) out8[k] = 0.0;
    if (count == 0) return;
    const double N = (double)(3u * (uint64_t)count);
    const double mse = e[0] / N;
    out8[0] = (double)count;
    out8[1] = mse;
    out8[2] = __builtin_sqrt(mse);
    out8[3] = e[1] / N;
    out8[4] = e[2] / N;
    out8[5] = e[3] / N;
    out8[6] = e[4];
    out8[7] = mse == 0.0 ? __builtin_inf() : 4.342944819032518 * rt_log((peak * peak) / mse); // 10 / ln 10, written once
}

// ---- rt_frame_noise_device: accumulators V, R (sums) and Rmax (a maximum) ----
constexpr int RT_NOISE_ACCS = 3;

// The per-channel variance of the mean of one pixel, as the denoisers' prepare step has it before it takes the largest channel
// (include/rt_amd.h "denoise": m_c = S_c / n, v_c = (Q_c - S_c * m_c) / (n - 1); "live denoise": v_c = M2_c / (n - 1)), then
// var_c = max(v_c, 0) / n with max(a, b) = (b > a ? b : a) — so that the largest var_c is prepare's V0 bit for bit.
RT_HD double rt_noise_variance(bool means, double first, double second, double dn) {
    double v;
    if (means) v = second / (dn - 1.0);
    else {
        const double m = first / dn;
        v = (second - first * m) / (dn - 1.0);
    }
    v = 0.0 > v ? 0.0 : v;
    return v / dn;
}

// One pixel: `first` its sums (means form: its running means), `second` its sums of squares (M2), n its sample count.  It counts iff
// n >= 2 and all six values are finite; per channel mean = "Input value" (S * (1.0 / (double)n); means form: S), var as above and
// rel = var / ((mean * mean) + eps); the entry is (var_r + var_g) + var_b, (rel_r + rel_g) + rel_b and the maximum of rel.
RT_HD void rt_noise_term(bool means, const double first[3], const double second[3], int32_t n, double eps, double e[RT_NOISE_ACCS], uint32_t *count) {
    *count = 0;
    for (int k = 0; k < RT_NOISE_ACCS; ++k) e[k] = 0.0;
    if (n < 2) return;
    for (int c = 0; c < 3; ++c)
        if (!rt_metrics_finite(first[c]) || !rt_metrics_finite(second[c])) return;
    const double dn = (double)n, inv = 1.0 / dn;
    double var[3], rel[3];
    for (int c = 0; c < 3; ++c) {
        const double mean = means ? first[c] : first[c] * inv;
        var[c] = rt_noise_variance(means, first[c], second[c], dn);
        rel[c] = var[c] / ((mean * mean) + eps);
    }
    e[0] = (var[0] + var[1]) + var[2];
    e[1] = (rel[0] + rel[1]) + rel[2];
    e[2] = rt_metrics_max(rt_metrics_max(rel[0], rel[1]), rel[2]);
    *count = 1;
}

RT_HD void rt_noise_combine(double a[RT_NOISE_ACCS], uint32_t *ca, const double b[RT_NOISE_ACCS], uint32_t cb) {
    a[0] = a[0] + b[0];
    a[1] = a[1] + b[1];
    a[2] = rt_metrics_max(a[2], b[2]);
    *ca = *ca + cb;
}

// out4 = count, mean_var, noise, max_noise; where nothing counts noise = max_noise = +inf (a stop test never passes) and mean_var = 0
RT_HD void rt_noise_result(const double e[RT_NOISE_ACCS], uint32_t count, double out4[4]) {
    out4[0] = 0.0;
    out4[1] = 0.0;
    out4[2] = out4[3] = __builtin_inf();
    if (count == 0) return;
    const double N = (double)(3u * (uint64_t)count);
    out4[0] = (double)count;
    out4[1] = e[0] / N;
    out4[2] = __builtin_sqrt(e[1] / N);
    out4[3] = __builtin_sqrt(e[2]);
}

} // namespace rtm

namespace rtmt {

constexpr int32_t LEVEL_BLOCK = 256;             // entries per block of the reduction tree (normative; tone mapping's)
constexpr int64_t MAX_PIXELS = (int64_t)1 << 27; // w * h must stay below this
constexpr int64_t ENTRY_BYTES = 48;              // a block's record in the workspace: up to five doubles and a 64-bit count

inline void defaults(rt_frame_error_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.eps = 1e-2;
    p.peak = 1.0;
}
inline void defaults(rt_frame_noise_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.eps = 1e-2;
}
template <class P>
inline bool size_known(uint32_t size) { return size >= 8 && size <= sizeof(P) && size % 8 == 0; }
inline bool error_size_known(uint32_t size) { return size_known<rt_frame_error_params>(size); }
inline bool noise_size_known(uint32_t size) { return size_known<rt_frame_noise_params>(size); }
// the caller's params over the defaults, as far as its struct goes; false: its struct_size is not one this library knows
template <class P>
inline bool resolve(const P *params, P &p) {
    defaults(p);
    if (!params) return true;
    if (!size_known<P>(params->struct_size)) return false;
    memcpy(&p, params, params->struct_size);
    return true;
}
inline bool frame_ok(int32_t w, int32_t h) { return w >= 1 && h >= 1 && (int64_t)w * h < MAX_PIXELS; }
inline bool positive_finite(double x) { return x > 0.0 && std::isfinite(x); }
inline int64_t level_blocks(int64_t n) { return (n + LEVEL_BLOCK - 1) / LEVEL_BLOCK; }
// the workspace: ENTRY_BYTES per block of every level, level 0's blocks first
inline int64_t workspace_bytes(int32_t w, int32_t h) {
    if (!frame_ok(w, h)) return -1;
    int64_t entries = 0;
    for (int64_t n = (int64_t)w * h;;) {
        n = level_blocks(n);
        entries += n;
        if (n == 1) break;
    }
    return entries * ENTRY_BYTES;
}
inline bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// rt_frame_error_device's and rth_frame_error's checks, in the header's order; `device`: the names carry the d_ prefix and the
// workspace is looked at.  Returns the message's tail, or null with `p` resolved.
inline const char *bad_error_argument(bool device, int32_t w, int32_t h, const double *values, int32_t spp, const double *ref, int32_t ref_spp,
                                      const rt_frame_error_params *params, const double *out8, const void *workspace, rt_frame_error_params &p) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (!values) return device ? "d_values is null" : "values is null";
    if (!ref) return device ? "d_ref is null" : "ref is null";
    if (!out8) return device ? "d_out8 is null" : "out8 is null";
    if (spp < 1) return "spp must be at least 1";
    if (ref_spp < 1) return "ref_spp must be at least 1";
    if (!resolve(params, p)) return "rt_frame_error_params.struct_size is not one this library knows";
    if (!positive_finite(p.eps)) return "eps must be a finite number > 0";
    if (!positive_finite(p.peak)) return "peak must be a finite number > 0";
    if (!device) return nullptr;
    if (!workspace) return "d_workspace is null";
    if (((uintptr_t)workspace & 15u) != 0) return "d_workspace must be 16-byte aligned";
    const size_t frame = (size_t)w * (size_t)h * 3u * sizeof(double);
    if (overlaps(out8, 8u * sizeof(double), values, frame)) return "d_out8 must not overlap d_values";
    if (overlaps(out8, 8u * sizeof(double), ref, frame)) return "d_out8 must not overlap d_ref";
    return nullptr;
}

inline const char *bad_noise_argument(bool device, int32_t w, int32_t h, int32_t form, const double *a, const double *b, int32_t n, const int32_t *spp_map,
                                      const rt_frame_noise_params *params, const double *out4, const void *workspace, rt_frame_noise_params &p) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (!a) return device ? "d_a is null" : "a is null";
    if (!b) return device ? "d_b is null" : "b is null";
    if (!out4) return device ? "d_out4 is null" : "out4 is null";
    if (n < 1) return "n must be at least 1";
    if (!resolve(params, p)) return "rt_frame_noise_params.struct_size is not one this library knows";
    if (form != RT_METRICS_SUMS && form != RT_METRICS_MEANS) return "form must be RT_METRICS_SUMS or RT_METRICS_MEANS (0..1)";
    if (form == RT_METRICS_MEANS && spp_map) return device ? "form RT_METRICS_MEANS takes no d_spp map" : "form RT_METRICS_MEANS takes no spp map";
    if (!positive_finite(p.eps)) return "eps must be a finite number > 0";
    if (!device) return nullptr;
    if (!workspace) return "d_workspace is null";
    if (((uintptr_t)workspace & 15u) != 0) return "d_workspace must be 16-byte aligned";
    const size_t frame = (size_t)w * (size_t)h * 3u * sizeof(double);
    if (overlaps(out4, 4u * sizeof(double), a, frame)) return "d_out4 must not overlap d_a";
    if (overlaps(out4, 4u * sizeof(double), b, frame)) return "d_out4 must not overlap d_b";
    return nullptr;
}

} // namespace rtmt
