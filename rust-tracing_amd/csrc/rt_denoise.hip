// rt_denoise.hip — the variance-guided à-trous denoiser of librt_amd (rt_denoise_device, include/rt_amd.h "denoise"): a prepare
// kernel that turns per-pixel sums and sums of squares into (mean, variance of the mean), and K edge-stopping wavelet iterations
// at strides 1, 2, 4, ... that ping-pong between the two halves of the caller's workspace.
//
// Everything is f64 in the header's operation order, each operation rounded on its own (the file is compiled with
// -ffp-contract=off and without fast-math: no FMA, IEEE division and square root), so a frame equals the numpy restatement in
// tests/denoise_helpers.py bit for bit.  Nothing here reads a scene; the render kernels (rt_kernel.hip) are not involved.
//
// Working set: one double4 (C_r, C_g, C_b, V) per pixel and half.  V = -1 marks a pixel that is not valid (fewer than two samples or
// a non-finite moment): it keeps its mean through every iteration and is never a tap.
// Shapes: a workgroup is 256 lanes = a 32 x 8 pixel tile, one pixel per lane, a row of the tile on 32 consecutive lanes (a wave covers
// two rows: its tap loads are two runs of 32 consecutive pixels, and its ds_read_b64 of 32 consecutive doubles per half-wave are
// conflict-free).  Strides 1 and 2 stage the tile plus a halo of 2 x stride pixels of (L, C, V) in the LDS, planes apart; out-of-frame
// halo pixels are staged as not valid, so the tap loop has no bounds test.  Strides >= 4 gather the taps from global memory (the
// working set stays in L2 / Infinity Cache at the project's frame sizes) and compute a tap's L from its C.
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int DN_TW = 32, DN_TH = 8, DN_THREADS = DN_TW * DN_TH;

// rt_kernel.hip's display_rgba8 (color_to_rgb(mean) with alpha 0xff, one little-endian word): the shared host / device code of
// rt_shared_math.h per value, so the bytes are rt_resolve_rgba8_device's
__device__ __forceinline__ uint32_t display_rgba8(double r, double g, double b) {
    return (uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(r)) | ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(g)) << 8) |
           ((uint32_t)rtm::rt_quantise(rtm::rt_gamma_encode(b)) << 16) | 0xff000000u;
}

__device__ __forceinline__ bool is_finite(double x) { return ((rtm::f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
__device__ __forceinline__ double luminance(double r, double g, double b) { return ((r + g) + b) / 3.0; }

// Prepare: m = S / n; a valid pixel's V0 = max(max(max(v_r, v_g), v_b), 0) / n with v_c = (Q_c - S_c * m_c) / (n - 1) and
// max(a, b) = b > a ? b : a; any other pixel's V = -1.  One thread per pixel.
__global__ __launch_bounds__(DN_THREADS) void denoise_prepare_kernel(int64_t n_pixels, const double *__restrict__ sum, const double *__restrict__ sum_sq,
                                                                      int32_t spp, const int32_t *__restrict__ spp_map, double4 *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (idx >= n_pixels) return;
    const int32_t n = spp_map ? spp_map[idx] : spp;
    const double dn = (double)n;
    const double s[3] = {sum[idx * 3 + 0], sum[idx * 3 + 1], sum[idx * 3 + 2]};
    const double q[3] = {sum_sq[idx * 3 + 0], sum_sq[idx * 3 + 1], sum_sq[idx * 3 + 2]};
    const double m[3] = {s[0] / dn, s[1] / dn, s[2] / dn};
    bool valid = n >= 2;
    for (int c = 0; c < 3; ++c) valid = valid && is_finite(s[c]) && is_finite(q[c]);
    double V = -1.0;
    if (valid) {
        double vmax = (q[0] - s[0] * m[0]) / (dn - 1.0);
        for (int c = 1; c < 3; ++c) {
            const double v = (q[c] - s[c] * m[c]) / (dn - 1.0);
            if (v > vmax) vmax = v;
        }
        if (0.0 > vmax) vmax = 0.0;
        V = vmax / dn;
    }
    out[idx] = make_double4(m[0], m[1], m[2], V);
}

struct Tap { double L, r, g, b, V; };

// where a lane's taps come from: the workgroup's staged tile (strides 1 and 2) ...
template <int S> struct LdsSource {
    static constexpr int HALO = 2 * S, PW = DN_TW + 2 * HALO, PH = DN_TH + 2 * HALO;
    const double *L, *r, *g, *b, *V;
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
        return true;
    }
};
// ... or global memory (strides >= 4)
struct GlobalSource {
    const double4 *in;
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
        const double4 c = in[(size_t)y * (size_t)w + (size_t)x];
        if (c.w < 0.0) return false;
        t.L = luminance(c.x, c.y, c.z); t.r = c.x; t.g = c.y; t.b = c.z; t.V = c.w;
        return true;
    }
};

// One iteration for one valid pixel (the header's "Iteration k"): the 3 x 3 prefilter of the variance, then the 25 taps in the order
// dy outer, dx inner.  Sums start from +0.0 and take one addition per tap used; nothing is reassociated.
template <class Source> __device__ __forceinline__ double4 filter_pixel(const Source &src, double Lp, double sigma, double eps) {
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
            const double x = __builtin_fabs(Lp - q.L) / den;
            const double t = 1.0 - x * x;
            const double e = t > 0.0 ? t * t : 0.0;
            const double wq = (h5[dy + 2] * h5[dx + 2]) * e;
            sw = sw + wq;
            sr = sr + wq * q.r;
            sg = sg + wq * q.g;
            sb = sb + wq * q.b;
            sv = sv + (wq * wq) * q.V;
        }
    return make_double4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// what an iteration writes for its pixel: the other half of the workspace, or — the last one — the caller's frame of means and,
// in the same pass, its display bytes
struct DenoiseOut {
    double4 *next;      // or null: the last iteration
    double *mean;       // 3 w h
    uint32_t *rgba;     // w h words, or null
};
__device__ __forceinline__ void store_pixel(const DenoiseOut &o, size_t pixel, const double4 &c) {
    if (o.next) {
        o.next[pixel] = c;
        return;
    }
    o.mean[pixel * 3u + 0u] = c.x; o.mean[pixel * 3u + 1u] = c.y; o.mean[pixel * 3u + 2u] = c.z;
    if (o.rgba) o.rgba[pixel] = display_rgba8(c.x, c.y, c.z);
}

template <int S>
__global__ __launch_bounds__(DN_THREADS) void atrous_lds_kernel(int32_t w, int32_t h, int32_t tiles_x, double sigma, double eps, const double4 *__restrict__ in, DenoiseOut out) {
    using Src = LdsSource<S>;
    constexpr int PW = Src::PW, PH = Src::PH, HALO = Src::HALO;
    __shared__ double sL[PH * PW], sR[PH * PW], sG[PH * PW], sB[PH * PW], sV[PH * PW];
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x; // a 1-D grid of tiles, row-major
    const int32_t x0 = tile_x * DN_TW - HALO, y0 = tile_y * DN_TH - HALO;
    for (int k = (int)threadIdx.x; k < PH * PW; k += DN_THREADS) {
        const int ly = k / PW, lx = k - ly * PW;
        const int32_t gx = x0 + lx, gy = y0 + ly;
        double4 c = make_double4(0.0, 0.0, 0.0, -1.0);
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) c = in[(size_t)gy * (size_t)w + (size_t)gx];
        sR[k] = c.x; sG[k] = c.y; sB[k] = c.z; sV[k] = c.w;
        sL[k] = luminance(c.x, c.y, c.z);
    }
    __syncthreads();
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int32_t px = tile_x * DN_TW + tx, py = tile_y * DN_TH + ty;
    if (px >= w || py >= h) return;
    const Src src{sL, sR, sG, sB, sV, (HALO + ty) * PW + HALO + tx};
    double4 c = make_double4(sR[src.centre], sG[src.centre], sB[src.centre], sV[src.centre]);
    if (!(c.w < 0.0)) c = filter_pixel(src, sL[src.centre], sigma, eps);
    store_pixel(out, (size_t)py * (size_t)w + (size_t)px, c);
}

__global__ __launch_bounds__(DN_THREADS) void atrous_global_kernel(int32_t w, int32_t h, int32_t tiles_x, int32_t stride, double sigma, double eps,
                                                                    const double4 *__restrict__ in, DenoiseOut out) {
    const int tx = (int)threadIdx.x & (DN_TW - 1), ty = (int)threadIdx.x / DN_TW;
    const int32_t tile_y = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int32_t)blockIdx.x - tile_y * tiles_x;
    const int32_t px = tile_x * DN_TW + tx, py = tile_y * DN_TH + ty;
    if (px >= w || py >= h) return;
    const size_t pixel = (size_t)py * (size_t)w + (size_t)px;
    double4 c = in[pixel];
    if (!(c.w < 0.0)) c = filter_pixel(GlobalSource{in, w, h, px, py, stride}, luminance(c.x, c.y, c.z), sigma, eps);
    store_pixel(out, pixel, c);
}

} // namespace

namespace rtk {

void launch_denoise_prepare(int64_t n_pixels, const double *sum, const double *sum_sq, int32_t spp, const int32_t *spp_map, void *half,
                            hipStream_t stream) {
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((n_pixels + DN_THREADS - 1) / DN_THREADS)), dim3(DN_THREADS), 0, stream,
                       n_pixels, sum, sum_sq, spp, spp_map, (double4 *)half);
}

void launch_denoise_atrous(int32_t w, int32_t h, int32_t stride, double sigma, double eps, const void *half_in, void *half_out,
                           double *mean_out, uint8_t *rgba8, hipStream_t stream) {
    const int32_t tiles_x = (w + DN_TW - 1) / DN_TW, tiles_y = (h + DN_TH - 1) / DN_TH;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y)), block(DN_THREADS); // (w * h < 2^27: fewer than 2^27 tiles)
    const DenoiseOut out{(double4 *)half_out, mean_out, (uint32_t *)rgba8};
    const double4 *in = (const double4 *)half_in;
    if (stride == 1) hipLaunchKernelGGL(atrous_lds_kernel<1>, grid, block, 0, stream, w, h, tiles_x, sigma, eps, in, out);
    else if (stride == 2) hipLaunchKernelGGL(atrous_lds_kernel<2>, grid, block, 0, stream, w, h, tiles_x, sigma, eps, in, out);
    else hipLaunchKernelGGL(atrous_global_kernel, grid, block, 0, stream, w, h, tiles_x, stride, sigma, eps, in, out);
}

} // namespace rtk
