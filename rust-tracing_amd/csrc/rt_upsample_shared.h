// rt_upsample_shared.h — guided upsampling (include/rt_amd.h "guided upsampling") as far as both libraries share it.
//   rtup::    host side only: the defaults, the struct sizes known, the checks in the header's order and the workspace's layout, so that
//             rt_upsample_device (rt_api.cpp) and its host mirror rth_upsample (host/capi.cpp) refuse the same things with the same words.
//   rtm::rt_upsample_*   the per-pixel functions, host and device: the prepare step of one low pixel and the 16 taps of one full-size
//             pixel, every operation rounded on its own, in the header's order.  The kernels (rt_upsample.hip) and the mirror run these
//             same functions, compiled without contraction on both sides, so their doubles agree bit for bit.
// Low records: three regions of 4 doubles per low pixel — (R_r, R_g, R_b, valid ? 1.0 : 0.0), (a_low_r, a_low_g, a_low_b, 0) and
// (g_low_r, g_low_g, g_low_b, 0) — so that a record is two aligned 16-byte accesses.  A guide's region is written and read only where
// that guide is given.
#pragma once
#include "rt_amd.h"
#include "rt_shared_math.h"

#include <cmath>
#include <cstring>

namespace rtm {

RT_HD bool rt_up_finite(double x) { return ((f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
RT_HD double rt_up_max(double a, double b) { return b > a ? b : a; } // the header's max(a, b)
RT_HD int32_t rt_up_low_size(int32_t n, int32_t F) { return (n + F - 1) / F; }

// the stop between a full guide value p and a low guide value q: d = max over the channels of |p_c - q_c|; z = d / sigma;
// t = 1 - z * z; t > 0 ? t * t : 0
RT_HD double rt_upsample_stop(const double p[3], double q0, double q1, double q2, double sigma) {
    const double d0 = __builtin_fabs(p[0] - q0), d1 = __builtin_fabs(p[1] - q1), d2 = __builtin_fabs(p[2] - q2);
    const double d = rt_up_max(rt_up_max(d0, d1), d2);
    const double z = d / sigma;
    const double t = 1.0 - z * z;
    return t > 0.0 ? t * t : 0.0;
}

// Prepare, one low pixel (I, J): its records rec_r, rec_a, rec_g (4 doubles each; rec_a / rec_g only with that guide).
RT_HD void rt_upsample_prepare(int32_t I, int32_t J, int32_t w, int32_t h, int32_t F, const double *low, double inv_spp, const double *albedo_sum,
                               double n_a, const double *edge_sum, double n_e, double albedo_floor, double *rec_r, double *rec_a, double *rec_g) {
    const int64_t lw = rt_up_low_size(w, F), q = (int64_t)J * lw + I;
    double c[3];
    bool valid = true;
    for (int k = 0; k < 3; ++k) {
        c[k] = low[q * 3 + k] * inv_spp;
        valid = valid && rt_up_finite(c[k]);
    }
    // the mean of a guide's full-size means over the block's in-frame pixels, rows outer
    auto block_mean = [&](const double *sum, double n, double *rec) {
        double acc[3] = {0.0, 0.0, 0.0};
        int32_t count = 0;
        for (int32_t y = F * J; y < F * J + F && y < h; ++y)
            for (int32_t x = F * I; x < F * I + F && x < w; ++x) {
                const double *v = sum + ((int64_t)y * w + x) * 3;
                for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (v[k] / n);
                ++count;
            }
        for (int k = 0; k < 3; ++k) {
            rec[k] = acc[k] / (double)count;
            valid = valid && rt_up_finite(rec[k]);
        }
        rec[3] = 0.0;
    };
    if (albedo_sum) {
        block_mean(albedo_sum, n_a, rec_a);
        for (int k = 0; k < 3; ++k) rec_r[k] = c[k] / rt_up_max(rec_a[k], albedo_floor);
    } else {
        for (int k = 0; k < 3; ++k) rec_r[k] = c[k];
    }
    if (edge_sum) block_mean(edge_sum, n_e, rec_g);
    rec_r[3] = valid ? 1.0 : 0.0;
}

// floor(t / d) for d > 0
RT_HD int32_t rt_up_floor_div(int32_t t, int32_t d) { return t >= 0 ? t / d : -((-t + d - 1) / d); }

// The low records as the regions hold them in memory (the kernels' direct form and the mirror).
struct UpsampleRegions {
    const double *r, *a, *g; // 4 doubles per low pixel each; a / g null without that guide
    int64_t lw;
    RT_HD bool valid(int32_t I, int32_t J) const { return r[((int64_t)J * lw + I) * 4 + 3] != 0.0; }
    RT_HD double R(int32_t I, int32_t J, int k) const { return r[((int64_t)J * lw + I) * 4 + k]; }
    RT_HD double A(int32_t I, int32_t J, int k) const { return a[((int64_t)J * lw + I) * 4 + k]; }
    RT_HD double G(int32_t I, int32_t J, int k) const { return g[((int64_t)J * lw + I) * 4 + k]; }
};

// One full-size pixel (x, y): the 16 taps, the stops and the output value.  ap and gp are the pixel's own full guide means (A / n_a,
// E / n_e; read only with that guide).  `rec` answers valid / R / A / G for a low pixel INSIDE the low frame; taps are asked for in
// the header's order, and `fallback` — the same interface — for the containing low pixel (x / F, y / F), which a tile's records may
// not hold.
template <bool HasA, bool HasG, class Records, class Fallback>
RT_HD void rt_upsample_pixel(int32_t x, int32_t y, int32_t F, int32_t lw, int32_t lh, const double ap[3], const double gp[3], double sigma_albedo,
                             double sigma_edge, double albedo_floor, const Records &rec, const Fallback &fallback, double out[3]) {
    const int32_t F2 = 2 * F, F4 = 4 * F;
    const int32_t tx = 2 * x + 1 - F, i0 = rt_up_floor_div(tx, F2), rx = tx - F2 * i0;
    const int32_t ty = 2 * y + 1 - F, j0 = rt_up_floor_div(ty, F2), ry = ty - F2 * j0;
    double sw = 0.0, sc[3] = {0.0, 0.0, 0.0};
    for (int dj = -1; dj <= 2; ++dj) {
        const int32_t J = j0 + dj;
        if (J < 0 || J >= lh) continue;
        const int32_t dy = F2 * dj - ry, ay = dy < 0 ? -dy : dy;
        const double wy = (double)(F4 - ay) / (double)F4;
        for (int di = -1; di <= 2; ++di) {
            const int32_t I = i0 + di;
            if (I < 0 || I >= lw) continue;
            if (!rec.valid(I, J)) continue;
            const int32_t dx = F2 * di - rx, ax = dx < 0 ? -dx : dx;
            const double wx = (double)(F4 - ax) / (double)F4;
            const double ws = wy * wx;
            double wt = ws;
            if constexpr (HasA && HasG) {
                const double ea = rt_upsample_stop(ap, rec.A(I, J, 0), rec.A(I, J, 1), rec.A(I, J, 2), sigma_albedo);
                const double eg = rt_upsample_stop(gp, rec.G(I, J, 0), rec.G(I, J, 1), rec.G(I, J, 2), sigma_edge);
                wt = ws * (ea * eg);
            } else if constexpr (HasA) {
                wt = ws * rt_upsample_stop(ap, rec.A(I, J, 0), rec.A(I, J, 1), rec.A(I, J, 2), sigma_albedo);
            } else if constexpr (HasG) {
                wt = ws * rt_upsample_stop(gp, rec.G(I, J, 0), rec.G(I, J, 1), rec.G(I, J, 2), sigma_edge);
            }
            sw = sw + wt;
            for (int k = 0; k < 3; ++k) sc[k] = sc[k] + (wt * rec.R(I, J, k));
        }
    }
    double r[3];
    if (sw > 0.0) {
        for (int k = 0; k < 3; ++k) r[k] = sc[k] / sw;
    } else {
        for (int k = 0; k < 3; ++k) r[k] = fallback.R(x / F, y / F, k);
    }
    for (int k = 0; k < 3; ++k) out[k] = HasA ? r[k] * rt_up_max(ap[k], albedo_floor) : r[k];
}

// color_to_rgb(out) with alpha 0xff, one little-endian word: the bytes of rt_resolve_rgba8_device
RT_HD uint32_t rt_upsample_rgba8(const double out[3]) {
    return (uint32_t)rt_quantise(rt_gamma_encode(out[0])) | ((uint32_t)rt_quantise(rt_gamma_encode(out[1])) << 8) |
           ((uint32_t)rt_quantise(rt_gamma_encode(out[2])) << 16) | 0xff000000u;
}

} // namespace rtm

namespace rtup {

constexpr int64_t MAX_PIXELS = (int64_t)1 << 27; // w * h must stay below this

inline void defaults(rt_upsample_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.factor = 2;
    p.sigma_edge = 0.5;
    p.sigma_albedo = 0.5;
    p.albedo_floor = 1e-3;
}
inline bool size_known(uint32_t size) { return size >= 8 && size <= sizeof(rt_upsample_params) && size % 8 == 0; }
// the caller's params over the defaults, as far as its struct goes; false: its struct_size is not one this library knows
inline bool resolve(const rt_upsample_params *params, rt_upsample_params &p) {
    defaults(p);
    if (!params) return true;
    if (!size_known(params->struct_size)) return false;
    memcpy(&p, params, params->struct_size);
    return true;
}
inline bool frame_ok(int32_t w, int32_t h) { return w >= 1 && h >= 1 && (int64_t)w * h < MAX_PIXELS; }
inline bool factor_ok(int32_t F) { return F >= 2 && F <= 4; }
inline const char *bad_field(const rt_upsample_params &p) {
    if (!factor_ok(p.factor)) return "factor must be 2, 3 or 4";
    if (!(p.sigma_edge > 0.0)) return "sigma_edge must be a number > 0";
    if (!(p.sigma_albedo > 0.0)) return "sigma_albedo must be a number > 0";
    if (!(p.albedo_floor > 0.0)) return "albedo_floor must be a number > 0";
    return nullptr;
}
inline int64_t low_pixels(int32_t w, int32_t h, int32_t F) { return (int64_t)rtm::rt_up_low_size(w, F) * rtm::rt_up_low_size(h, F); }
// the workspace: three regions (R and the valid flag, the low albedo, the low edge guide) of 4 doubles per LOW pixel
inline int64_t region_bytes(int32_t w, int32_t h, int32_t F) { return low_pixels(w, h, F) * 4 * (int64_t)sizeof(double); }
inline int64_t workspace_bytes(int32_t w, int32_t h, int32_t F) { return frame_ok(w, h) && factor_ok(F) ? 3 * region_bytes(w, h, F) : -1; }
// the checks the device call and the mirror share, in the header's order up to the params (device: the pointers are d_low, d_mean_out
// and d_workspace; the mirror has low and out_mean and no workspace); null: all fine, and p is resolved
inline const char *bad_argument(bool device, int32_t w, int32_t h, const void *low, const void *out, const void *workspace, int32_t spp,
                                const void *albedo, int32_t albedo_spp, const void *edge, int32_t edge_spp, const rt_upsample_params *params,
                                rt_upsample_params &p) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (!low) return device ? "d_low is null" : "low is null";
    if (!out) return device ? "d_mean_out is null" : "out_mean is null";
    if (device && !workspace) return "d_workspace is null";
    if (spp < 1) return "spp must be at least 1";
    if (albedo && albedo_spp < 1) return "albedo_spp must be at least 1 with an albedo guide";
    if (edge && edge_spp < 1) return "edge_spp must be at least 1 with an edge guide";
    if (!resolve(params, p)) return "rt_upsample_params.struct_size is not one this library knows";
    return bad_field(p);
}
inline bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}
// the input d_mean_out (3 * w * h doubles) overlaps, as the message's tail; null: none
inline const char *bad_overlap(bool device, int32_t w, int32_t h, int32_t F, const void *out, const void *low, const void *albedo, const void *edge) {
    const size_t full = (size_t)w * (size_t)h * 24u, small = (size_t)low_pixels(w, h, F) * 24u;
    if (overlap(out, full, low, small)) return device ? "d_mean_out must not overlap d_low" : "out_mean must not overlap low";
    if (albedo && overlap(out, full, albedo, full)) return device ? "d_mean_out must not overlap d_albedo_sum" : "out_mean must not overlap albedo_sum";
    if (edge && overlap(out, full, edge, full)) return device ? "d_mean_out must not overlap d_edge_sum" : "out_mean must not overlap edge_sum";
    return nullptr;
}

} // namespace rtup
