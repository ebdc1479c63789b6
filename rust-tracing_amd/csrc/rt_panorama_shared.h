// rt_panorama_shared.h — equirectangular panoramas (include/rt_amd.h "panoramas"), the text both sides of the boundary compile:
//   rtpn::pixel           the per-pixel body: an output pixel's direction from the tables, its face, its four taps and the bilinear
//                         blend of a pixel's three channels.  The kernel (rt_panorama.hip, one thread per output pixel) and the host
//                         mirror (rth_panorama, host/capi.cpp) run it word for word, without contraction on either side, so the mirror
//                         holds the device's bits.  No transcendental, no square root: the only division is by the largest component.
//   the host-side part    the checks in the header's order, so that rt_panorama_device (rt_api.cpp) and rth_panorama refuse the same
//                         things with the same words; the cube-face cameras and the tables, which no device ever sees being made.
#pragma once
#include "rt_amd.h"
#include "rt_shared_math.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#include <cstddef>
#endif

namespace rtpn {

constexpr int32_t MAX_FACE = 16384;

// min(max((int32_t)floor(v), 0), hi) for every v, a NaN included (it gives 0): below 0 the floor is clamped away, from 0 on the
// conversion's truncation is the floor, and a v of hi or more never reaches the conversion
RT_HD int32_t texel_floor(double v, int32_t hi) { return !(v >= 0.0) ? 0 : v >= (double)hi ? hi : (int32_t)v; }
RT_HD double unit_clamp(double t) { return t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t; }

// One output pixel: sl, cl the column's table entries, sp, cp the row's; `faces` the six frames of 3 F F doubles, face-major.
RT_HD void pixel(double sl, double cl, double sp, double cp, const double *faces, int32_t F, int32_t g, double inv_spp, double out[3]) {
    // Direction
    const double dx = cp * sl, dy = sp, dz = -(cp * cl);
    const double ax = dx < 0.0 ? -dx : dx, ay = dy < 0.0 ? -dy : dy, az = dz < 0.0 ? -dz : dz;
    // Face, and the components along its right and up axes (a signed component each: exact)
    int32_t face;
    double m, da, db;
    if (ax >= ay && ax >= az) {
        m = ax;
        if (dx > 0.0) { face = 0; da = dz; db = dy; }
        else { face = 1; da = -dz; db = dy; }
    } else if (ay >= az) {
        m = ay;
        if (dy > 0.0) { face = 2; da = dx; db = dz; }
        else { face = 3; da = dx; db = -dz; }
    } else {
        m = az;
        if (dz > 0.0) { face = 4; da = -dx; db = dy; }
        else { face = 5; da = dx; db = dy; }
    }
    const double a = da / m, b = db / m;
    // Texel coordinates
    const double s = (double)(F - 2 * g) * 0.5, c = (double)F * 0.5 - 0.5;
    const double as = a * s, bs = b * s;
    const double x = as + c, y = c - bs;
    const int32_t x0 = texel_floor(x, F - 2), y0 = texel_floor(y, F - 2);
    const double fx = unit_clamp(x - (double)x0), fy = unit_clamp(y - (double)y0);
    // Taps and output
    const double *t00 = faces + ((int64_t)face * F * F + (int64_t)y0 * F + x0) * 3;
    const double *t01 = t00 + (int64_t)F * 3;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        const double T00 = t00[k] * inv_spp, T10 = t00[3 + k] * inv_spp, T01 = t01[k] * inv_spp, T11 = t01[3 + k] * inv_spp;
        const double dt = T10 - T00, db2 = T11 - T01;
        const double pt = dt * fx, pb = db2 * fx;
        const double top = T00 + pt, bot = T01 + pb;
        const double dv = bot - top;
        const double pv = dv * fy;
        out[k] = top + pv;
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side ----

constexpr int64_t MAX_PIXELS = (int64_t)1 << 27;  // w * h must stay below this

// face_size and guard, as rt_camera_cube_faces and the resampler refuse them, in the header's order; null: all fine
inline const char *bad_face(int32_t face_size, int32_t guard) {
    if (face_size < 2 || face_size > MAX_FACE) return "face_size must be from 2 to 16384";
    if (guard < 0) return "guard must not be negative";
    if (face_size - 2 * (int64_t)guard < 1) return "face_size - 2 * guard must be at least 1";
    return nullptr;
}
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}
// the checks the device call and the mirror share, in the header's order (device: d_tables, d_faces, d_mean_out; the mirror: tables,
// faces, out_mean); null: all fine
inline const char *bad_argument(bool device, int32_t w, int32_t h, const void *tables, const void *faces, int32_t face_size, int32_t guard,
                                int32_t spp, const void *out) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (const char *bad = bad_face(face_size, guard)) return bad;
    if (!tables) return device ? "d_tables is null" : "tables is null";
    if (!faces) return device ? "d_faces is null" : "faces is null";
    if (!out) return device ? "d_mean_out is null" : "out_mean is null";
    if (spp < 1) return "spp must be at least 1";
    const size_t frame = (size_t)w * (size_t)h * 3u * sizeof(double);
    if (ranges_overlap(out, frame, tables, (2u * (size_t)w + 2u * (size_t)h) * sizeof(double)))
        return device ? "d_mean_out must not overlap d_tables" : "out_mean must not overlap tables";
    if (ranges_overlap(out, frame, faces, 6u * 3u * (size_t)face_size * (size_t)face_size * sizeof(double)))
        return device ? "d_mean_out must not overlap d_faces" : "out_mean must not overlap faces";
    return nullptr;
}

// The six cameras of "panoramas", "Cube-face cameras": plain f64, each operation rounded on its own.  The caller has checked F and g.
inline void cube_faces(const rt_camera &like, const double center[3], int32_t F, int32_t g, rt_camera out[6]) {
    // forward n, up u, right r = n x u, as (axis, sign)
    static const int8_t AXES[6][3][2] = {{{0, 1}, {1, 1}, {2, 1}},   {{0, -1}, {1, 1}, {2, -1}}, {{1, 1}, {2, 1}, {0, 1}},
                                         {{1, -1}, {2, -1}, {0, 1}}, {{2, 1}, {1, 1}, {0, -1}},  {{2, -1}, {1, 1}, {0, 1}}};
    const double inner = (double)(F - 2 * g);
    const double delta = 2.0 / inner;
    const double hh = (double)F / inner;
    const double half = 0.5 * delta;
    const double e = half - hh;
    const double c[3] = {center ? center[0] : like.center.x, center ? center[1] : like.center.y, center ? center[2] : like.center.z};
    for (int f = 0; f < 6; ++f) {
        double du[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
        const int8_t(*ax)[2] = AXES[f];
        t[ax[0][0]] = (double)ax[0][1];           // n
        t[ax[2][0]] = ax[2][1] > 0 ? e : -e;      // + r * e
        t[ax[1][0]] = ax[1][1] > 0 ? -e : e;      // - u * e
        du[ax[2][0]] = ax[2][1] > 0 ? delta : -delta;
        dv[ax[1][0]] = ax[1][1] > 0 ? -delta : delta;
        rt_camera cam = like;
        cam.image_width = F;
        cam.image_height = F;
        cam.center = rt_vec3{c[0], c[1], c[2]};
        cam.pixel00_loc = rt_vec3{c[0] + t[0], c[1] + t[1], c[2] + t[2]};
        cam.pixel_delta_u = rt_vec3{du[0], du[1], du[2]};
        cam.pixel_delta_v = rt_vec3{dv[0], dv[1], dv[2]};
        cam.defocus_angle = 0.0;
        cam.defocus_disk_u = rt_vec3{0.0, 0.0, 0.0};
        cam.defocus_disk_v = rt_vec3{0.0, 0.0, 0.0};
        out[f] = cam;
    }
}

// The tables of "panoramas", "Tables": 2 w column entries, then 2 h row entries.
inline void tables(int32_t w, int32_t h, double *t) {
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    for (int32_t i = 0; i < w; ++i) {
        const double q = ((double)i + 0.5) / (double)w;
        const double lambda = (q - 0.5) * two_pi;
        t[2 * (size_t)i] = std::sin(lambda);
        t[2 * (size_t)i + 1] = std::cos(lambda);
    }
    double *rows = t + 2 * (size_t)w;
    for (int32_t j = 0; 2 * j < h; ++j) {   // the upper half and the middle row; the lower half is its mirror image
        const double q = ((double)j + 0.5) / (double)h;
        const double phi = (0.5 - q) * pi;
        const double s = std::sin(phi), c = std::cos(phi);
        rows[2 * (size_t)j] = s;
        rows[2 * (size_t)j + 1] = c;
        const size_t k = (size_t)(h - 1 - j);
        if ((int32_t)k != j) {
            rows[2 * k] = -s;
            rows[2 * k + 1] = c;
        }
    }
}

// the whole frame on the host, pixel after pixel
inline void resample(int32_t w, int32_t h, const double *t, const double *faces, int32_t F, int32_t g, int32_t spp, double *out) {
    const double inv_spp = 1.0 / (double)spp;
    const double *rows = t + 2 * (size_t)w;
    for (int32_t j = 0; j < h; ++j)
        for (int32_t i = 0; i < w; ++i)
            pixel(t[2 * (size_t)i], t[2 * (size_t)i + 1], rows[2 * (size_t)j], rows[2 * (size_t)j + 1], faces, F, g, inv_spp,
                  out + ((size_t)j * (size_t)w + (size_t)i) * 3u);
}
#endif

} // namespace rtpn
