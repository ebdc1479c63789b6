// rt_denoise.hip — the à-trous denoisers of librt_amd, one template in two instantiations: the variance-guided filter
// (rt_denoise_device, include/rt_amd.h "denoise") and, with Guided, the albedo-guided one (rt_denoise_albedo_device, "albedo-guided
// denoise").  A prepare kernel turns per-pixel sums and sums of squares into (mean, variance of the mean) — Guided: divides the mean
// by the first-hit albedo (floored) first, which leaves the irradiance — and K edge-stopping wavelet iterations at strides 1, 2, 4, ...
// ping-pong between the two halves of the caller's workspace.  They stop at luminance edges and, Guided, at edges of the albedo as
// well: one more factor per tap; the last Guided iteration multiplies the albedo back in.  What only the guided filter does sits
// behind `if constexpr (Guided)`, so the plain instantiations hold none of it and the two cannot drift apart.  Prepare has a second
// compile-time parameter, the input form: sums and sums of squares, or (Means: rt_denoise_mean_device, rt_denoise_albedo_mean_device)
// the live route's running means and Welford's M2; the iterations do not know which it was.  A third prepare, a tile kernel, serves
// frames of so few samples that M2 says nothing (rt_denoise_mean_spatial_device, "spatial variance"): it takes V0 from the spread of the
// neighbouring pixels' values — and, with an edge guide, of those of its own surface only.  The guide is a small compile-time mode (DN_PLAIN, DN_ALBEDO, DN_EDGES, DN_BOTH below): an EDGE guide
// (rt_denoise_guided_device, "edge-guided denoise") is a guide frame that contributes one more stop factor per tap and nothing else —
// no division in prepare, nothing multiplied back — alone, where it reuses the albedo mode's guide region, planes and loads, or beside
// the albedo guide, with a fourth region of the workspace, three more staged planes (eleven: 40 x 16 x 11 x 8 B = 56 320 B at stride
// 2, two workgroups per CU) and a third double4 per gathered tap.  The plain and albedo instantiations hold none of it: their
// instruction streams are what they were before the mode existed.
//
// Everything is f64 in the header's operation order, each operation rounded on its own (the file is compiled with
// -ffp-contract=off and without fast-math: no FMA, IEEE division and square root), so a frame equals the numpy restatement in
// tests/denoise_helpers.py (Guided: tests/albedo_helpers.py) bit for bit, and the guided filter is the plain one where the albedo is 1
// everywhere.  Nothing here reads a scene; the render kernels (rt_kernel.hip) are not involved.
//
// Working set: one double4 (C_r, C_g, C_b, V) per pixel and half.  V = -1 marks a pixel that is not valid (fewer than two samples or
// a non-finite moment): it keeps its mean through every iteration and is never a tap.  Guided: a third region that prepare writes
// once, the guide, one double4 (a_r, a_g, a_b, 0) per pixel, the un-floored albedo means.  The divisor max(a, floor) is three
// compares: the last iteration makes it again from the guide instead of keeping it.
// Shapes: a workgroup is 256 lanes = a 32 x 8 pixel tile, one pixel per lane, a row of the tile on 32 consecutive lanes (a wave covers
// two rows: its tap loads are two runs of 32 consecutive pixels, and its ds_read_b64 of 32 consecutive doubles per half-wave are
// conflict-free); the grid's first dimension is the frame's tiles, row-major, its second the view: a launch filters a stack of grid.y
// frames (rt_denoise_views_device, rt_denoise_albedo_views_device) that lie one behind the other in every buffer, and a workgroup
// addresses its pixels as `first pixel of its view + pixel of the frame` while every bounds test stays the frame's own, so no tap, halo
// pixel or window member is ever a neighbouring view's.  The single-frame entry points launch grid.y = 1 and add zero.
// Strides 1 and 2 stage the tile plus a halo of 2 x stride pixels in the LDS, planes
// apart: (L, C x 3, V), five planes, and Guided (a x 3) as well, eight (40 x 16 x 8 x 8 B = 40 960 B at stride 2); out-of-frame halo
// pixels are staged as not valid, so the tap loop has no bounds test.  Strides >= 4 gather the taps from global memory (the working
// set stays in L2 / Infinity Cache at the project's frame sizes; Guided: two double4 per tap) and compute a tap's L from its C.
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>
#include <type_traits>

namespace {

constexpr int DN_TW = 32, DN_TH = 8, DN_THREADS = DN_TW * DN_TH;

// the guides of an instantiation, a small mode: none, the demodulating albedo guide, an edge guide (rt_denoise_guided_device: one stop
// factor per tap and nothing else), or both.  Edges alone reuses what the albedo mode has for its guide — the third region of the
// workspace, the planes P_AR .. P_AB, a tap's (ar, ag, ab) — for the edge guide's means, without the albedo mode's divisions; beside
// the albedo guide the edge guide has a region, three planes and three tap fields (er, eg, eb) of its own.
constexpr int DN_PLAIN = 0, DN_ALBEDO = 1, DN_EDGES = 2, DN_BOTH = 3;
constexpr bool demodulates(int mode) { return (mode & DN_ALBEDO) != 0; }
constexpr bool has_edges(int mode) { return (mode & DN_EDGES) != 0; }

// what a kernel gets of the guides: the launcher's description(s), or — the plain instantiations — nothing, so no argument of theirs is live
struct NoGuide {};
struct BothGuides { rtk::DenoiseGuide albedo; rtk::DenoiseEdge edge; };
template <int Mode>
using GuideOf = std::conditional_t<Mode == DN_PLAIN, NoGuide,
                                   std::conditional_t<Mode == DN_ALBEDO, rtk::DenoiseGuide, std::conditional_t<Mode == DN_EDGES, rtk::DenoiseEdge, BothGuides>>>;
__device__ __forceinline__ const rtk::DenoiseGuide &albedo_of(const rtk::DenoiseGuide &g) { return g; }
__device__ __forceinline__ const rtk::DenoiseGuide &albedo_of(const BothGuides &g) { return g.albedo; }
__device__ __forceinline__ const rtk::DenoiseEdge &edge_of(const rtk::DenoiseEdge &g) { return g; }
__device__ __forceinline__ const rtk::DenoiseEdge &edge_of(const BothGuides &g) { return g.edge; }
// the first guide (what the third region, P_AR .. P_AB and (ar, ag, ab) hold): its region and the width of its stop
__device__ __forceinline__ double4 *first_region(const rtk::DenoiseGuide &g) { return g.region; }
__device__ __forceinline__ double4 *first_region(const rtk::DenoiseEdge &g) { return g.region; }
__device__ __forceinline__ double4 *first_region(const BothGuides &g) { return g.albedo.region; }
__device__ __forceinline__ double first_sigma(const rtk::DenoiseGuide &g) { return g.sigma_albedo; }
__device__ __forceinline__ double first_sigma(const rtk::DenoiseEdge &g) { return g.sigma_edge; }
__device__ __forceinline__ double first_sigma(const BothGuides &g) { return g.albedo.sigma_albedo; }

// rt_kernel.hip's display_rgba8 (color_to_rgb(mean) with alpha 0xff, one little-endian word): the shared host / device code of
// rt_shared_math.h per value, so the bytes are rt_resolve_rgba8_device's
__device__ __forceinline__ uint32_t display_rgba8(double r, double g, double b) {
    return (uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(r)) | ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(g)) << 8) |
           ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(b)) << 16) | 0xff000000u;
}

__device__ __forceinline__ bool is_finite(double x) { return ((rtm::f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
__device__ __forceinline__ double luminance(double r, double g, double b) { return ((r + g) + b) / 3.0; }
__device__ __forceinline__ double max_ab(double a, double b) { return b > a ? b : a; } // the header's max(a, b)

// Prepare: m = S / n; a valid pixel's V0 = max(max(max(v_r, v_g), v_b), 0) / n with v_c = (Q_c - S_c * m_c) / (n - 1) and C0 = m; any
// other pixel's C = m and V = -1.  Guided: a = A / n_a is the guide, a pixel with a non-finite A is not valid either, and a valid
// pixel's d = max(a, floor), C0 = m / d, V0 from u_c = v_c / (d_c * d_c) in v_c's place.  One thread per pixel.
// Means (rt_denoise_mean_device, rt_denoise_albedo_mean_device: the live route's frames): `sum` holds the running means m and `sum_sq`
// Welford's M2 after n = spp samples of every pixel (no map), the guide's frame the albedo means a: nothing is divided by a count, and
// v_c = M2_c / (n - 1).  Everything else is the sums form's, which holds none of this.
// An edge guide (Mode with DN_EDGES): g = E / n_e is written to its region, a pixel with a non-finite E is not valid, and C0 and V0
// are not touched by it.  Means (rt_denoise_guided_mean_device): the guide's frame holds means, g = E with nothing divided, as a is.
template <int Mode, bool Means>
__global__ __launch_bounds__(DN_THREADS) void denoise_prepare_kernel(int64_t n_pixels, const double *__restrict__ sum, const double *__restrict__ sum_sq,
                                                                      int32_t spp, const int32_t *__restrict__ spp_map, GuideOf<Mode> gd,
                                                                      double4 *__restrict__ out) {
    constexpr bool Guided = demodulates(Mode);
    const int64_t in_frame = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (in_frame >= n_pixels) return;
    const size_t idx = (size_t)blockIdx.y * (size_t)n_pixels + (size_t)in_frame; // the pixel in the stack of views (n_pixels: one frame's)
    const int32_t n = spp_map ? spp_map[idx] : spp;
    const double dn = (double)n;
    const double s[3] = {sum[idx * 3 + 0], sum[idx * 3 + 1], sum[idx * 3 + 2]};
    const double q[3] = {sum_sq[idx * 3 + 0], sum_sq[idx * 3 + 1], sum_sq[idx * 3 + 2]};
    double A[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
    if constexpr (Guided)
        for (int k = 0; k < 3; ++k) {
            A[k] = albedo_of(gd).albedo_sum[idx * 3 + k];
            if constexpr (Means) a[k] = A[k];
            else a[k] = A[k] / albedo_of(gd).albedo_spp;
        }
    double E[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
    if constexpr (has_edges(Mode))
        for (int k = 0; k < 3; ++k) {
            E[k] = edge_of(gd).edge_sum[idx * 3 + k];
            if constexpr (Means) g[k] = E[k];
            else g[k] = E[k] / edge_of(gd).edge_spp;
        }
    double c[3] = {s[0], s[1], s[2]};
    if constexpr (!Means)
        for (int k = 0; k < 3; ++k) c[k] = s[k] / dn;
    bool valid = n >= 2;
    for (int k = 0; k < 3; ++k) valid = valid && is_finite(s[k]) && is_finite(q[k]) && is_finite(A[k]);
    if constexpr (has_edges(Mode))
        for (int k = 0; k < 3; ++k) valid = valid && is_finite(E[k]);
    double V = -1.0;
    if (valid) {
        double vmax = 0.0;
        for (int k = 0; k < 3; ++k) {
            double v;
            if constexpr (Means) v = q[k] / (dn - 1.0);
            else v = (q[k] - s[k] * c[k]) / (dn - 1.0);
            if constexpr (Guided) {
                const double d = max_ab(a[k], albedo_of(gd).albedo_floor);
                v = v / (d * d);
                c[k] = c[k] / d;
            }
            vmax = k == 0 ? v : max_ab(vmax, v);
        }
        vmax = max_ab(vmax, 0.0);
        V = vmax / dn;
    }
    out[idx] = make_double4(c[0], c[1], c[2], V);
    if constexpr (Guided) albedo_of(gd).region[idx] = make_double4(a[0], a[1], a[2], 0.0);
    if constexpr (has_edges(Mode)) edge_of(gd).region[idx] = make_double4(g[0], g[1], g[2], 0.0);
}

// The spatial prepare (rt_denoise_mean_spatial_device, rt_denoise_albedo_mean_spatial_device below their threshold; include/rt_amd.h
// "spatial variance"): a frame of so few samples that M2 says nothing gets its V0 from the spread of C0 over the valid pixels of the
// (2R + 1)^2 window around each pixel, C0 = m or, Guided, m / max(a, floor).  It takes the elementwise prepare's place on that route and
// writes what it writes: (C0, V0) into the first half and, Guided, the guide; d_m2 is not read.  The workgroup stages its tile plus a
// halo of R pixels, planes apart: (C0 x 3, valid), 38 x 14 x 4 x 8 B = 17 024 B at R = 3; the guided division is done once per staged
// pixel, and out-of-frame halo pixels are staged as not valid, so the window loops have no bounds test.  A pixel that is not valid is
// staged with C0 = m, which its own lane writes back.  Each lane then makes the definition's two passes over the staged window, dy
// outer and dx inner: the sum and the count of the members, then the sum of the squared differences from their mean.  A pixel that
// is not a member is skipped: nothing is added for it.
// An edge guide (Mode with DN_EDGES; rt_denoise_guided_mean_spatial_device, "edge guide on every route") restricts the window to the
// centre pixel's own surface: three more planes hold the guide's means g (seven: 38 x 14 x 7 x 8 B = 29 792 B at R = 3), a pixel with
// a non-finite g is not valid, and a valid window pixel is a member only where the iterations' edge stop would let it through,
// tg = 1 - (dg / sigma_edge)^2 > 0 with dg the largest channel difference from the centre's g.  P_OK is tested first, so the staged
// guide of an out-of-frame or invalid pixel is never read.  Both passes make the test: nothing of the first is kept for the second.
// The plain and albedo instantiations hold none of it.
template <int R, int Mode> struct SpatialTile {
    static constexpr int PW = DN_TW + 2 * R, PH = DN_TH + 2 * R, PLANE = PH * PW;
    enum { P_R, P_G, P_B, P_OK, P_ER, P_EG, P_EB, PLANES = has_edges(Mode) ? 7 : 4 };
    // q, a valid pixel at k of the staged planes, is of the centre's surface (the centre's guide is e)
    static __device__ __forceinline__ bool member(const double *staged, int k, const double (&e)[3], double sigma_edge) {
        const double dg = max_ab(max_ab(__builtin_fabs(e[0] - staged[P_ER * PLANE + k]), __builtin_fabs(e[1] - staged[P_EG * PLANE + k])),
                                 __builtin_fabs(e[2] - staged[P_EB * PLANE + k]));
        const double z = dg / sigma_edge;
        const double tg = 1.0 - z * z;
        return tg > 0.0;
    }
};
template <int R, int Mode>
__global__ __launch_bounds__(DN_THREADS) void denoise_prepare_spatial_kernel(int32_t w, int32_t h, int32_t tiles_x, const double *__restrict__ mean,
                                                                              GuideOf<Mode> gd, double4 *__restrict__ out) {
    constexpr bool Guided = demodulates(Mode), Edges = has_edges(Mode);
    using T = SpatialTile<R, Mode>;
    constexpr int PW = T::PW, PLANE = T::PLANE;
    __shared__ double staged[T::PLANES * PLANE];
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x; // a 1-D grid of tiles, row-major
    const int32_t x0 = tile_x * DN_TW - R, y0 = tile_y * DN_TH - R;
    for (int k = (int)threadIdx.x; k < PLANE; k += DN_THREADS) {
        const int ly = k / PW, lx = k - ly * PW;
        const int32_t gx = x0 + lx, gy = y0 + ly;
        double c[3] = {0.0, 0.0, 0.0};
        [[maybe_unused]] double e[3] = {0.0, 0.0, 0.0};
        bool valid = false;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = ((size_t)gy * (size_t)w + (size_t)gx) * 3u;
            valid = true;
            for (int ch = 0; ch < 3; ++ch) {
                c[ch] = mean[g + ch];
                valid = valid && is_finite(c[ch]);
            }
            if constexpr (Edges)
                for (int ch = 0; ch < 3; ++ch) {
                    e[ch] = edge_of(gd).edge_sum[g + ch];
                    valid = valid && is_finite(e[ch]);
                }
            if constexpr (Guided) {
                double a[3];
                for (int ch = 0; ch < 3; ++ch) {
                    a[ch] = albedo_of(gd).albedo_sum[g + ch];
                    valid = valid && is_finite(a[ch]);
                }
                if (valid)
                    for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] / max_ab(a[ch], albedo_of(gd).albedo_floor);
            }
        }
        staged[T::P_R * PLANE + k] = c[0]; staged[T::P_G * PLANE + k] = c[1]; staged[T::P_B * PLANE + k] = c[2];
        staged[T::P_OK * PLANE + k] = valid ? 1.0 : 0.0;
        if constexpr (Edges) { staged[T::P_ER * PLANE + k] = e[0]; staged[T::P_EG * PLANE + k] = e[1]; staged[T::P_EB * PLANE + k] = e[2]; }
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int32_t px = tile_x * DN_TW + tx, py = tile_y * DN_TH + ty;
    if (px >= w || py >= h) return;
    const int centre = (R + ty) * PW + R + tx;
    const size_t pixel = (size_t)py * (size_t)w + (size_t)px;
    double V = -1.0;
    if (staged[T::P_OK * PLANE + centre] != 0.0) {
        double cnt = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0}, mu[3];
        [[maybe_unused]] double e[3] = {0.0, 0.0, 0.0}; // the centre's guide
        if constexpr (Edges) { e[0] = staged[T::P_ER * PLANE + centre]; e[1] = staged[T::P_EG * PLANE + centre]; e[2] = staged[T::P_EB * PLANE + centre]; }
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int k = centre + dy * PW + dx;
                if (staged[T::P_OK * PLANE + k] == 0.0) continue;
                if constexpr (Edges)
                    if (!T::member(staged, k, e, edge_of(gd).sigma_edge)) continue;
                cnt = cnt + 1.0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) s1[ch] = s1[ch] + staged[ch * PLANE + k];
            }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) mu[ch] = s1[ch] / cnt;
        // (a compiler-only fence: the second pass tests the window's members again.  Without it the first pass's (2R + 1)^2 wave masks
        // are kept for the second: 106 SGPRs with 10 / 6 of them spilled at R = 3 against 46 / 34 and none with it — DESIGN.md section 5
        // "Spatial variance" has both tables)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int dy = -R; dy <= R; ++dy)
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int k = centre + dy * PW + dx;
                if (staged[T::P_OK * PLANE + k] == 0.0) continue;
                if constexpr (Edges)
                    if (!T::member(staged, k, e, edge_of(gd).sigma_edge)) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double t = staged[ch * PLANE + k] - mu[ch];
                    s2[ch] = s2[ch] + t * t;
                }
            }
        double v[3] = {0.0, 0.0, 0.0};
        if (cnt >= 2.0)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = s2[ch] / (cnt - 1.0);
        V = max_ab(max_ab(v[0], v[1]), v[2]);
    }
    out[pixel] = make_double4(staged[T::P_R * PLANE + centre], staged[T::P_G * PLANE + centre], staged[T::P_B * PLANE + centre], V);
    if constexpr (Guided) {
        const rtk::DenoiseGuide &ag = albedo_of(gd);
        ag.region[pixel] = make_double4(ag.albedo_sum[pixel * 3u + 0u], ag.albedo_sum[pixel * 3u + 1u], ag.albedo_sum[pixel * 3u + 2u], 0.0);
    }
    if constexpr (Edges) // (the staged guide is the frame's entry itself, valid or not)
        edge_of(gd).region[pixel] = make_double4(staged[T::P_ER * PLANE + centre], staged[T::P_EG * PLANE + centre], staged[T::P_EB * PLANE + centre], 0.0);
}

// (ar, ag, ab: the tap's first guide, the albedo means or — edges alone — the edge guide's means; er, eg, eb: the edge guide's means
// beside an albedo guide; neither is set by an instantiation without it)
struct Tap { double L, r, g, b, V, ar, ag, ab, er, eg, eb; };

// where a lane's taps come from: the workgroup's staged tile (strides 1 and 2) ...
template <int S, int Mode> struct LdsSource {
    static constexpr bool Guided = Mode != DN_PLAIN, Second = Mode == DN_BOTH;
    static constexpr int HALO = 2 * S, PW = DN_TW + 2 * HALO, PH = DN_TH + 2 * HALO, PLANE = PH * PW;
    enum { P_L, P_R, P_G, P_B, P_V, P_AR, P_AG, P_AB, P_ER, P_EG, P_EB, PLANES = Second ? 11 : Guided ? 8 : 5 };
    const double *staged; // PLANES planes of PLANE doubles
    int centre;           // the lane's own pixel in a plane
    __device__ __forceinline__ double at(int plane, int k) const { return staged[plane * PLANE + k]; }
    __device__ __forceinline__ bool variance(int dx, int dy, double &v) const {
        v = at(P_V, centre + dy * PW + dx);
        return !(v < 0.0);
    }
    __device__ __forceinline__ bool tap(int dx, int dy, Tap &t) const {
        const int k = centre + (dy * PW + dx) * S;
        t.V = at(P_V, k);
        if (t.V < 0.0) return false;
        t.L = at(P_L, k); t.r = at(P_R, k); t.g = at(P_G, k); t.b = at(P_B, k);
        if constexpr (Guided) { t.ar = at(P_AR, k); t.ag = at(P_AG, k); t.ab = at(P_AB, k); }
        if constexpr (Second) { t.er = at(P_ER, k); t.eg = at(P_EG, k); t.eb = at(P_EB, k); }
        return true;
    }
};
// ... or global memory (strides >= 4)
struct NoRegion {};
template <int Mode> struct GlobalSource {
    static constexpr bool Guided = Mode != DN_PLAIN, Second = Mode == DN_BOTH;
    const double4 *in, *guide; // (guide: the first guide's region; Guided only)
    int32_t w, h, px, py, stride;
    std::conditional_t<Second, const double4 *, NoRegion> edge; // (the edge guide's region beside an albedo guide)
    __device__ __forceinline__ bool variance(int dx, int dy, double &v) const {
        const int32_t x = px + dx, y = py + dy;
        if (x < 0 || x >= w || y < 0 || y >= h) return false;
        v = in[(size_t)y * (size_t)w + (size_t)x].w;
        return !(v < 0.0);
    }
    __device__ __forceinline__ bool tap(int dx, int dy, Tap &t) const {
        const int32_t x = px + dx * stride, y = py + dy * stride;
        if (x < 0 || x >= w || y < 0 || y >= h) return false;
        const size_t k = (size_t)y * (size_t)w + (size_t)x;
        const double4 c = in[k];
        if (c.w < 0.0) return false;
        t.L = luminance(c.x, c.y, c.z); t.r = c.x; t.g = c.y; t.b = c.z; t.V = c.w;
        if constexpr (Guided) {
            const double4 a = guide[k];
            t.ar = a.x; t.ag = a.y; t.ab = a.z;
        }
        if constexpr (Second) {
            const double4 g = edge[k];
            t.er = g.x; t.eg = g.y; t.eb = g.z;
        }
        return true;
    }
};

// One iteration for one valid pixel p (the header's "Iteration k"), which leaves with its new C and V: the 3 x 3 prefilter of the
// variance, then the 25 taps in the order dy outer, dx inner, each weighted by the luminance stop e and, Guided, the albedo stop ea.
// Sums start from +0.0 and take one addition per tap used; nothing is reassociated.
// An edge guide's stop eg has ea's form over the edge guide's means and sigma_edge: alone it is the one further factor, e * eg; beside
// the albedo guide the weight is (e * ea) * eg.
template <int Mode, class Source>
__device__ __forceinline__ void filter_pixel(const Source &src, Tap &p, double sigma, double eps, const GuideOf<Mode> &gd) {
    constexpr bool Guided = Mode != DN_PLAIN;
    const double g3[3] = {0.25, 0.5, 0.25};
    double gs = 0.0, ws = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            double v;
            if (!src.variance(dx, dy, v)) continue;
            const double k = g3[dy + 1] * g3[dx + 1];
            gs = gs + k * v;
            ws = ws + k;
        }
    const double G = gs / ws;
    const double sd = __builtin_sqrt(G);
    const double den = sigma * sd + eps;
    const double h5[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            Tap q;
            if (!src.tap(dx, dy, q)) continue;
            const double x = __builtin_fabs(p.L - q.L) / den;
            const double t = 1.0 - x * x;
            double e = t > 0.0 ? t * t : 0.0;
            if constexpr (Guided) {
                const double da = max_ab(max_ab(__builtin_fabs(p.ar - q.ar), __builtin_fabs(p.ag - q.ag)), __builtin_fabs(p.ab - q.ab));
                const double y = da / first_sigma(gd);
                const double ta = 1.0 - y * y;
                const double ea = ta > 0.0 ? ta * ta : 0.0;
                e = e * ea;
            }
            if constexpr (Mode == DN_BOTH) {
                const double dg = max_ab(max_ab(__builtin_fabs(p.er - q.er), __builtin_fabs(p.eg - q.eg)), __builtin_fabs(p.eb - q.eb));
                const double z = dg / gd.edge.sigma_edge;
                const double tg = 1.0 - z * z;
                const double eg = tg > 0.0 ? tg * tg : 0.0;
                e = e * eg;
            }
            const double wq = (h5[dy + 2] * h5[dx + 2]) * e;
            sw = sw + wq;
            sr = sr + wq * q.r;
            sg = sg + wq * q.g;
            sb = sb + wq * q.b;
            sv = sv + (wq * wq) * q.V;
        }
    p.r = sr / sw; p.g = sg / sw; p.b = sb / sw; p.V = sv / (sw * sw);
}

// what an iteration writes for its pixel: the other half of the workspace, or — the last one — the caller's frame of means (Guided: a
// valid pixel's irradiance times its divisor max(a, floor); any other pixel's mean as it is) and, in the same pass, its display bytes
struct DenoiseOut {
    double4 *next;      // or null: the last iteration
    double *mean;       // 3 w h
    uint32_t *rgba;     // w h words, or null
};
template <int Mode>
__device__ __forceinline__ void store_pixel(const DenoiseOut &o, size_t pixel, Tap p, const GuideOf<Mode> &gd) {
    if (o.next) {
        o.next[pixel] = make_double4(p.r, p.g, p.b, p.V);
        return;
    }
    if constexpr (demodulates(Mode)) // (an edge guide multiplies nothing back in)
        if (!(p.V < 0.0)) {
            p.r = p.r * max_ab(p.ar, albedo_of(gd).albedo_floor);
            p.g = p.g * max_ab(p.ag, albedo_of(gd).albedo_floor);
            p.b = p.b * max_ab(p.ab, albedo_of(gd).albedo_floor);
        }
    o.mean[pixel * 3u + 0u] = p.r; o.mean[pixel * 3u + 1u] = p.g; o.mean[pixel * 3u + 2u] = p.b;
    if (o.rgba) o.rgba[pixel] = display_rgba8(p.r, p.g, p.b);
}

template <int S, int Mode>
__global__ __launch_bounds__(DN_THREADS) void atrous_lds_kernel(int32_t w, int32_t h, int32_t tiles_x, double sigma, double eps, GuideOf<Mode> gd,
                                                                 const double4 *__restrict__ in, DenoiseOut out) {
    using Src = LdsSource<S, Mode>;
    constexpr bool Guided = Src::Guided, Second = Src::Second;
    constexpr int PW = Src::PW, PLANE = Src::PLANE, HALO = Src::HALO;
    __shared__ double staged[Src::PLANES * PLANE];
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x; // grid.x: tiles, row-major
    const size_t view = (size_t)blockIdx.y * ((size_t)w * (size_t)h); // grid.y: the view; its first pixel in every buffer
    const int32_t x0 = tile_x * DN_TW - HALO, y0 = tile_y * DN_TH - HALO;
    for (int k = (int)threadIdx.x; k < PLANE; k += DN_THREADS) {
        const int ly = k / PW, lx = k - ly * PW;
        const int32_t gx = x0 + lx, gy = y0 + ly;
        double4 c = make_double4(0.0, 0.0, 0.0, -1.0), a = make_double4(0.0, 0.0, 0.0, 0.0);
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = view + (size_t)gy * (size_t)w + (size_t)gx;
            c = in[g];
            if constexpr (Guided) a = first_region(gd)[g];
        }
        staged[Src::P_R * PLANE + k] = c.x; staged[Src::P_G * PLANE + k] = c.y; staged[Src::P_B * PLANE + k] = c.z; staged[Src::P_V * PLANE + k] = c.w;
        staged[Src::P_L * PLANE + k] = luminance(c.x, c.y, c.z);
        if constexpr (Guided) { staged[Src::P_AR * PLANE + k] = a.x; staged[Src::P_AG * PLANE + k] = a.y; staged[Src::P_AB * PLANE + k] = a.z; }
        if constexpr (Second) {
            double4 e = make_double4(0.0, 0.0, 0.0, 0.0);
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) e = gd.edge.region[view + (size_t)gy * (size_t)w + (size_t)gx];
            staged[Src::P_ER * PLANE + k] = e.x; staged[Src::P_EG * PLANE + k] = e.y; staged[Src::P_EB * PLANE + k] = e.z;
        }
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int32_t px = tile_x * DN_TW + tx, py = tile_y * DN_TH + ty;
    if (px >= w || py >= h) return;
    const Src src{staged, (HALO + ty) * PW + HALO + tx};
    const int k = src.centre;
    Tap p;
    p.L = src.at(Src::P_L, k); p.r = src.at(Src::P_R, k); p.g = src.at(Src::P_G, k); p.b = src.at(Src::P_B, k); p.V = src.at(Src::P_V, k);
    if constexpr (Guided) { p.ar = src.at(Src::P_AR, k); p.ag = src.at(Src::P_AG, k); p.ab = src.at(Src::P_AB, k); }
    if constexpr (Second) { p.er = src.at(Src::P_ER, k); p.eg = src.at(Src::P_EG, k); p.eb = src.at(Src::P_EB, k); }
    if (!(p.V < 0.0)) filter_pixel<Mode>(src, p, sigma, eps, gd);
    store_pixel<Mode>(out, view + (size_t)py * (size_t)w + (size_t)px, p, gd);
}

template <int Mode>
__global__ __launch_bounds__(DN_THREADS) void atrous_global_kernel(int32_t w, int32_t h, int32_t tiles_x, int32_t stride, double sigma, double eps,
                                                                    GuideOf<Mode> gd, const double4 *__restrict__ in, DenoiseOut out) {
    constexpr bool Guided = Mode != DN_PLAIN, Second = Mode == DN_BOTH;
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x;
    const int32_t px = tile_x * DN_TW + tx, py = tile_y * DN_TH + ty;
    if (px >= w || py >= h) return;
    const size_t view = (size_t)blockIdx.y * ((size_t)w * (size_t)h), pixel = (size_t)py * (size_t)w + (size_t)px; // (grid.y: the view)
    const double4 *guide = nullptr;
    if constexpr (Guided) guide = first_region(gd) + view;
    in += view; // the taps index their own view's frame
    const double4 c = in[pixel];
    Tap p;
    p.L = luminance(c.x, c.y, c.z); p.r = c.x; p.g = c.y; p.b = c.z; p.V = c.w;
    if constexpr (Guided) {
        const double4 a = guide[pixel];
        p.ar = a.x; p.ag = a.y; p.ab = a.z;
    }
    if constexpr (Second) {
        const double4 *edge = gd.edge.region + view;
        const double4 g = edge[pixel];
        p.er = g.x; p.eg = g.y; p.eb = g.z;
        if (!(p.V < 0.0)) filter_pixel<Mode>(GlobalSource<Mode>{in, guide, w, h, px, py, stride, edge}, p, sigma, eps, gd);
    } else if (!(p.V < 0.0)) filter_pixel<Mode>(GlobalSource<Mode>{in, guide, w, h, px, py, stride}, p, sigma, eps, gd);
    store_pixel<Mode>(out, view + pixel, p, gd);
}

template <int Mode, bool Means>
void launch_prepare(int64_t n_pixels, int32_t n_views, const double *sum, const double *sum_sq, int32_t spp, const int32_t *spp_map, const GuideOf<Mode> &gd,
                    void *half, hipStream_t stream) {
    hipLaunchKernelGGL((denoise_prepare_kernel<Mode, Means>), dim3((unsigned)((n_pixels + DN_THREADS - 1) / DN_THREADS), (unsigned)n_views), dim3(DN_THREADS), 0,
                       stream, n_pixels, sum, sum_sq, spp, spp_map, gd, (double4 *)half);
}

template <int R, int Mode>
void launch_prepare_spatial(int32_t w, int32_t h, const double *mean, const GuideOf<Mode> &gd, void *half, hipStream_t stream) {
    const int32_t tiles_x = (w + DN_TW - 1) / DN_TW, tiles_y = (h + DN_TH - 1) / DN_TH;
    hipLaunchKernelGGL((denoise_prepare_spatial_kernel<R, Mode>), dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(DN_THREADS), 0, stream, w, h,
                       tiles_x, mean, gd, (double4 *)half);
}
template <int R>
void launch_prepare_spatial(int32_t w, int32_t h, const double *mean, const rtk::DenoiseGuide *guide, const rtk::DenoiseEdge *edge, void *half, hipStream_t stream) {
    if (guide && edge) launch_prepare_spatial<R, DN_BOTH>(w, h, mean, BothGuides{*guide, *edge}, half, stream);
    else if (edge) launch_prepare_spatial<R, DN_EDGES>(w, h, mean, *edge, half, stream);
    else if (guide) launch_prepare_spatial<R, DN_ALBEDO>(w, h, mean, *guide, half, stream);
    else launch_prepare_spatial<R, DN_PLAIN>(w, h, mean, NoGuide{}, half, stream);
}

template <int Mode>
void launch_atrous(int32_t w, int32_t h, int32_t n_views, int32_t stride, double sigma, double eps, const GuideOf<Mode> &gd, const void *half_in, const DenoiseOut &out,
                   hipStream_t stream) {
    const int32_t tiles_x = (w + DN_TW - 1) / DN_TW, tiles_y = (h + DN_TH - 1) / DN_TH;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), (unsigned)n_views), block(DN_THREADS); // (w * h < 2^27: fewer than 2^27 tiles; n_views <= 65535)
    const double4 *in = (const double4 *)half_in;
    if (stride == 1) hipLaunchKernelGGL((atrous_lds_kernel<1, Mode>), grid, block, 0, stream, w, h, tiles_x, sigma, eps, gd, in, out);
    else if (stride == 2) hipLaunchKernelGGL((atrous_lds_kernel<2, Mode>), grid, block, 0, stream, w, h, tiles_x, sigma, eps, gd, in, out);
    else hipLaunchKernelGGL(atrous_global_kernel<Mode>, grid, block, 0, stream, w, h, tiles_x, stride, sigma, eps, gd, in, out);
}

} // namespace

namespace rtk {

void launch_denoise_prepare(int64_t n_pixels, int32_t n_views, const double *sum, const double *sum_sq, int32_t spp, const int32_t *spp_map, const DenoiseGuide *guide,
                            bool means, void *half, hipStream_t stream, const DenoiseEdge *edge) {
    if (means) { // (a uniform count: the means form has no map)
        if (guide && edge) launch_prepare<DN_BOTH, true>(n_pixels, n_views, sum, sum_sq, spp, nullptr, BothGuides{*guide, *edge}, half, stream);
        else if (edge) launch_prepare<DN_EDGES, true>(n_pixels, n_views, sum, sum_sq, spp, nullptr, *edge, half, stream);
        else if (guide) launch_prepare<DN_ALBEDO, true>(n_pixels, n_views, sum, sum_sq, spp, nullptr, *guide, half, stream);
        else launch_prepare<DN_PLAIN, true>(n_pixels, n_views, sum, sum_sq, spp, nullptr, NoGuide{}, half, stream);
    } else if (guide && edge) launch_prepare<DN_BOTH, false>(n_pixels, n_views, sum, sum_sq, spp, spp_map, BothGuides{*guide, *edge}, half, stream);
    else if (edge) launch_prepare<DN_EDGES, false>(n_pixels, n_views, sum, sum_sq, spp, spp_map, *edge, half, stream);
    else if (guide) launch_prepare<DN_ALBEDO, false>(n_pixels, n_views, sum, sum_sq, spp, spp_map, *guide, half, stream);
    else launch_prepare<DN_PLAIN, false>(n_pixels, n_views, sum, sum_sq, spp, spp_map, NoGuide{}, half, stream);
}

void launch_denoise_prepare_spatial(int32_t w, int32_t h, int32_t radius, const double *mean, const DenoiseGuide *guide, void *half, hipStream_t stream,
                                    const DenoiseEdge *edge) {
    if (radius == 1) launch_prepare_spatial<1>(w, h, mean, guide, edge, half, stream);
    else if (radius == 2) launch_prepare_spatial<2>(w, h, mean, guide, edge, half, stream);
    else launch_prepare_spatial<3>(w, h, mean, guide, edge, half, stream); // (the caller has checked 1..3)
}

void launch_denoise_atrous(int32_t w, int32_t h, int32_t n_views, int32_t stride, double sigma, double eps, const DenoiseGuide *guide, const void *half_in,
                           void *half_out, double *mean_out, uint8_t *rgba8, hipStream_t stream, const DenoiseEdge *edge) {
    const DenoiseOut out{(double4 *)half_out, mean_out, (uint32_t *)rgba8};
    if (guide && edge) launch_atrous<DN_BOTH>(w, h, n_views, stride, sigma, eps, BothGuides{*guide, *edge}, half_in, out, stream);
    else if (edge) launch_atrous<DN_EDGES>(w, h, n_views, stride, sigma, eps, *edge, half_in, out, stream);
    else if (guide) launch_atrous<DN_ALBEDO>(w, h, n_views, stride, sigma, eps, *guide, half_in, out, stream);
    else launch_atrous<DN_PLAIN>(w, h, n_views, stride, sigma, eps, NoGuide{}, half_in, out, stream);
}

} // namespace rtk
