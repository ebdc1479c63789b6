// rt_denoise_albedo.hip — the albedo-guided à-trous denoiser of librt_amd (rt_denoise_albedo_device, include/rt_amd.h "albedo-guided
// denoise"): a prepare kernel that divides the frame of means by the first-hit albedo (floored) and turns the moments into (irradiance,
// variance of its mean), and K edge-stopping wavelet iterations at strides 1, 2, 4, ... that stop at luminance edges of the irradiance
// and at edges of the albedo; the last one multiplies the albedo back in.  rt_denoise.hip's shapes and tap loop with one more factor
// per tap; that file is not touched, so the plain filter's kernels compile as before.
//
// Everything is f64 in the header's operation order, each operation rounded on its own (the file is compiled with
// -ffp-contract=off and without fast-math: no FMA, IEEE division and square root), so a frame equals the numpy restatement in
// tests/albedo_helpers.py bit for bit — and rt_denoise_device's where the albedo is 1 everywhere.
//
// Working set: the two halves of rt_denoise.hip (one double4 (C_r, C_g, C_b, V) per pixel, V = -1: not valid) and a third region that
// prepare writes once: the guide, one double4 (a_r, a_g, a_b, 0) per pixel, the un-floored albedo means.  The divisor max(a, floor) is
// three compares: the last iteration makes it again from the guide instead of keeping it.
// Shapes: 256 lanes = a 32 x 8 tile, a 1-D grid of tiles; strides 1 and 2 stage tile + halo of (L, C x 3, V, a x 3) in the LDS, eight
// planes apart (40 x 16 x 8 x 8 B = 40 960 B at stride 2), out-of-frame halo pixels staged as not valid; strides >= 4 gather from
// global memory (two double4 per tap).
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int DA_TW = 32, DA_TH = 8, DA_THREADS = DA_TW * DA_TH;

// rt_kernel.hip's display_rgba8: the bytes are rt_resolve_rgba8_device's
__device__ __forceinline__ uint32_t display_rgba8(double r, double g, double b) {
    return (uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(r)) | ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(g)) << 8) |
           ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(b)) << 16) | 0xff000000u;
}

__device__ __forceinline__ bool is_finite(double x) { return ((rtm::f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
__device__ __forceinline__ double luminance(double r, double g, double b) { return ((r + g) + b) / 3.0; }
__device__ __forceinline__ double max_ab(double a, double b) { return b > a ? b : a; } // the header's max(a, b)

// Prepare: m = S / n, a = A / n_a; a valid pixel's d = max(a, floor), C0 = m / d, V0 = max(max(max(u_r, u_g), u_b), 0) / n with
// u_c = ((Q_c - S_c * m_c) / (n - 1)) / (d_c * d_c); any other pixel's C = m and V = -1.  One thread per pixel.
__global__ __launch_bounds__(DA_THREADS) void albedo_prepare_kernel(int64_t n_pixels, const double *__restrict__ sum, const double *__restrict__ sum_sq,
                                                                     int32_t spp, const int32_t *__restrict__ spp_map,
                                                                     const double *__restrict__ albedo_sum, double albedo_spp, double albedo_floor,
                                                                     double4 *__restrict__ out, double4 *__restrict__ guide) {
    const int64_t idx = (int64_t)blockIdx.x * DA_THREADS + threadIdx.x;
    if (idx >= n_pixels) return;
    const int32_t n = spp_map ? spp_map[idx] : spp;
    const double dn = (double)n;
    const double s[3] = {sum[idx * 3 + 0], sum[idx * 3 + 1], sum[idx * 3 + 2]};
    const double q[3] = {sum_sq[idx * 3 + 0], sum_sq[idx * 3 + 1], sum_sq[idx * 3 + 2]};
    const double A[3] = {albedo_sum[idx * 3 + 0], albedo_sum[idx * 3 + 1], albedo_sum[idx * 3 + 2]};
    const double a[3] = {A[0] / albedo_spp, A[1] / albedo_spp, A[2] / albedo_spp};
    double c[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
    bool valid = n >= 2;
    for (int k = 0; k < 3; ++k) valid = valid && is_finite(s[k]) && is_finite(q[k]) && is_finite(A[k]);
    double V = -1.0;
    if (valid) {
        double umax = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double m = c[k];
            const double d = max_ab(a[k], albedo_floor);
            const double v = (q[k] - s[k] * m) / (dn - 1.0);
            const double u = v / (d * d);
            umax = k == 0 ? u : max_ab(umax, u);
            c[k] = m / d;
        }
        umax = max_ab(umax, 0.0);
        V = umax / dn;
    }
    out[idx] = make_double4(c[0], c[1], c[2], V);
    guide[idx] = make_double4(a[0], a[1], a[2], 0.0);
}

struct Tap { double L, r, g, b, V, ar, ag, ab; };

// where a lane's taps come from: the workgroup's staged tile (strides 1 and 2) ...
template <int S> struct LdsSource {
    static constexpr int HALO = 2 * S, PW = DA_TW + 2 * HALO, PH = DA_TH + 2 * HALO;
    const double *L, *r, *g, *b, *V, *ar, *ag, *ab;
    int centre; // the lane's own pixel in the staged planes
    __device__ __forceinline__ bool variance(int dx, int dy, double &v) const {
        v = V[centre + dy * PW + dx];
        return !(v < 0.0);
    }
    __device__ __forceinline__ bool tap(int dx, int dy, Tap &t) const {
        const int k = centre + (dy * PW + dx) * S;
        t.V = V[k];
        if (t.V < 0.0) return false;
        t.L = L[k]; t.r = r[k]; t.g = g[k]; t.b = b[k];
        t.ar = ar[k]; t.ag = ag[k]; t.ab = ab[k];
        return true;
    }
};
// ... or global memory (strides >= 4)
struct GlobalSource {
    const double4 *in, *guide;
    int32_t w, h, px, py, stride;
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
        const double4 a = guide[k];
        t.L = luminance(c.x, c.y, c.z); t.r = c.x; t.g = c.y; t.b = c.z; t.V = c.w;
        t.ar = a.x; t.ag = a.y; t.ab = a.z;
        return true;
    }
};

struct FilterParams { double sigma, eps, sigma_albedo, albedo_floor; };

// One iteration for one valid pixel (the header's "Iteration k"): the 3 x 3 prefilter of the variance, then the 25 taps in the order
// dy outer, dx inner, each weighted by the luminance stop e and the albedo stop ea.  Sums start from +0.0 and take one addition per
// tap used; nothing is reassociated.
template <class Source>
__device__ __forceinline__ double4 filter_pixel(const Source &src, double Lp, double apr, double apg, double apb, const FilterParams &f) {
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
    const double den = f.sigma * sd + f.eps;
    const double h5[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            Tap q;
            if (!src.tap(dx, dy, q)) continue;
            const double x = __builtin_fabs(Lp - q.L) / den;
            const double t = 1.0 - x * x;
            const double e = t > 0.0 ? t * t : 0.0;
            const double da = max_ab(max_ab(__builtin_fabs(apr - q.ar), __builtin_fabs(apg - q.ag)), __builtin_fabs(apb - q.ab));
            const double y = da / f.sigma_albedo;
            const double ta = 1.0 - y * y;
            const double ea = ta > 0.0 ? ta * ta : 0.0;
            const double wq = (h5[dy + 2] * h5[dx + 2]) * (e * ea);
            sw = sw + wq;
            sr = sr + wq * q.r;
            sg = sg + wq * q.g;
            sb = sb + wq * q.b;
            sv = sv + (wq * wq) * q.V;
        }
    return make_double4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// what an iteration writes for its pixel: the other half of the workspace, or — the last one — the caller's frame of means (a valid
// pixel's irradiance times its divisor max(a, floor); any other pixel's mean as it is) and, in the same pass, its display bytes
struct AlbedoOut {
    double4 *next;      // or null: the last iteration
    double *mean;       // 3 w h
    uint32_t *rgba;     // w h words, or null
};
__device__ __forceinline__ void store_pixel(const AlbedoOut &o, size_t pixel, double4 c, double ar, double ag, double ab, double albedo_floor) {
    if (o.next) {
        o.next[pixel] = c;
        return;
    }
    if (!(c.w < 0.0)) {
        c.x = c.x * max_ab(ar, albedo_floor);
        c.y = c.y * max_ab(ag, albedo_floor);
        c.z = c.z * max_ab(ab, albedo_floor);
    }
    o.mean[pixel * 3u + 0u] = c.x; o.mean[pixel * 3u + 1u] = c.y; o.mean[pixel * 3u + 2u] = c.z;
    if (o.rgba) o.rgba[pixel] = display_rgba8(c.x, c.y, c.z);
}

template <int S>
__global__ __launch_bounds__(DA_THREADS) void albedo_atrous_lds_kernel(int32_t w, int32_t h, int32_t tiles_x, FilterParams f, const double4 *__restrict__ in,
                                                                        const double4 *__restrict__ guide, AlbedoOut out) {
    using Src = LdsSource<S>;
    constexpr int PW = Src::PW, PH = Src::PH, HALO = Src::HALO;
    __shared__ double sL[PH * PW], sR[PH * PW], sG[PH * PW], sB[PH * PW], sV[PH * PW], sAr[PH * PW], sAg[PH * PW], sAb[PH * PW];
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x; // a 1-D grid of tiles, row-major
    const int32_t x0 = tile_x * DA_TW - HALO, y0 = tile_y * DA_TH - HALO;
    for (int k = (int)threadIdx.x; k < PH * PW; k += DA_THREADS) {
        const int ly = k / PW, lx = k - ly * PW;
        const int32_t gx = x0 + lx, gy = y0 + ly;
        double4 c = make_double4(0.0, 0.0, 0.0, -1.0), a = make_double4(0.0, 0.0, 0.0, 0.0);
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = (size_t)gy * (size_t)w + (size_t)gx;
            c = in[g];
            a = guide[g];
        }
        sR[k] = c.x; sG[k] = c.y; sB[k] = c.z; sV[k] = c.w;
        sL[k] = luminance(c.x, c.y, c.z);
        sAr[k] = a.x; sAg[k] = a.y; sAb[k] = a.z;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DA_TW - 1), ty = (int)threadIdx.x / DA_TW;
    const int32_t px = tile_x * DA_TW + tx, py = tile_y * DA_TH + ty;
    if (px >= w || py >= h) return;
    const Src src{sL, sR, sG, sB, sV, sAr, sAg, sAb, (HALO + ty) * PW + HALO + tx};
    const double ar = sAr[src.centre], ag = sAg[src.centre], ab = sAb[src.centre];
    double4 c = make_double4(sR[src.centre], sG[src.centre], sB[src.centre], sV[src.centre]);
    if (!(c.w < 0.0)) c = filter_pixel(src, sL[src.centre], ar, ag, ab, f);
    store_pixel(out, (size_t)py * (size_t)w + (size_t)px, c, ar, ag, ab, f.albedo_floor);
}

__global__ __launch_bounds__(DA_THREADS) void albedo_atrous_global_kernel(int32_t w, int32_t h, int32_t tiles_x, int32_t stride, FilterParams f,
                                                                           const double4 *__restrict__ in, const double4 *__restrict__ guide, AlbedoOut out) {
    const int tx = (int)threadIdx.x & (DA_TW - 1), ty = (int)threadIdx.x / DA_TW;
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x;
    const int32_t px = tile_x * DA_TW + tx, py = tile_y * DA_TH + ty;
    if (px >= w || py >= h) return;
    const size_t pixel = (size_t)py * (size_t)w + (size_t)px;
    double4 c = in[pixel];
    const double4 a = guide[pixel];
    if (!(c.w < 0.0)) c = filter_pixel(GlobalSource{in, guide, w, h, px, py, stride}, luminance(c.x, c.y, c.z), a.x, a.y, a.z, f);
    store_pixel(out, pixel, c, a.x, a.y, a.z, f.albedo_floor);
}

} // namespace

namespace rtk {

void launch_denoise_albedo_prepare(int64_t n_pixels, const double *sum, const double *sum_sq, int32_t spp, const int32_t *spp_map,
                                   const double *albedo_sum, int32_t albedo_spp, double albedo_floor, void *half, void *guide, hipStream_t stream) {
    hipLaunchKernelGGL(albedo_prepare_kernel, dim3((unsigned)((n_pixels + DA_THREADS - 1) / DA_THREADS)), dim3(DA_THREADS), 0, stream,
                       n_pixels, sum, sum_sq, spp, spp_map, albedo_sum, (double)albedo_spp, albedo_floor, (double4 *)half, (double4 *)guide);
}

void launch_denoise_albedo_atrous(int32_t w, int32_t h, int32_t stride, double sigma, double eps, double sigma_albedo, double albedo_floor,
                                  const void *half_in, const void *guide, void *half_out, double *mean_out, uint8_t *rgba8, hipStream_t stream) {
    const int32_t tiles_x = (w + DA_TW - 1) / DA_TW, tiles_y = (h + DA_TH - 1) / DA_TH;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y)), block(DA_THREADS); // (w * h < 2^27: fewer than 2^27 tiles)
    const AlbedoOut out{(double4 *)half_out, mean_out, (uint32_t *)rgba8};
    const FilterParams f{sigma, eps, sigma_albedo, albedo_floor};
    const double4 *in = (const double4 *)half_in, *gd = (const double4 *)guide;
    if (stride == 1) hipLaunchKernelGGL(albedo_atrous_lds_kernel<1>, grid, block, 0, stream, w, h, tiles_x, f, in, gd, out);
    else if (stride == 2) hipLaunchKernelGGL(albedo_atrous_lds_kernel<2>, grid, block, 0, stream, w, h, tiles_x, f, in, gd, out);
    else hipLaunchKernelGGL(albedo_atrous_global_kernel, grid, block, 0, stream, w, h, tiles_x, stride, f, in, gd, out);
}

} // namespace rtk
