// rt_tonemap.hip — the tone-mapping output stage of librt_amd (rt_tonemap_device, rt_log_average_luminance_device; include/rt_amd.h
// "tone mapping").  Two kinds of kernel, scene-free and apart from the render kernels as rt_denoise.hip is:
//   the level kernel reduces one level of the log-average tree: 256 entries per block, one per thread, through the normative
//     `for stride = 128 .. 1: e[i] = e[i] + e[i + stride]` — strides 128 and 64 through the LDS, and once a single wave64 is left the
//     strides 32 .. 1 through cross-lane moves, lane i taking lane i + stride's value: the same pairs in the same order.  Level 0 makes
//     each pixel's term from the frame; every block writes its (T, count) to the workspace, and the block of a one-block level also
//     writes the four result doubles.  No atomics: the sum's order is the header's whatever the launch shape.
//   the value kernels are the existing resolve kernels with the exposure and the operator in front of the gamma: one thread per value
//     for RGB8, one per pixel and one packed 32-bit store for RGBA8.  With auto-exposure they read `scale` from the workspace, where the
//     last level left it, so the whole call stays on the stream.
// Everything is f64 in the header's order, each operation rounded on its own (-ffp-contract=off, no fast-math, IEEE division); the
// per-value arithmetic is rt_shared_math.h's, which the host mirror (rth_tonemap) runs too, so device and host bytes are identical.
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int TM_THREADS = 256; // the tree's block: normative, not a tuning choice

// One level.  First: entry idx is pixel idx's term, from values (3 per pixel) and its sample count (the uniform reciprocal inv_spp, or
// 1 / spp_map[idx]); otherwise entry idx is in[idx].  n_in entries; the grid is ceil(n_in / 256) blocks, the entries beyond n_in are
// the padding (+0.0, count 0).  out4 is written by block 0 of a one-block grid only.
template <bool First>
__global__ __launch_bounds__(TM_THREADS) void tonemap_level_kernel(uint32_t n_in, const double *__restrict__ values, double inv_spp,
                                                                   const int32_t *__restrict__ spp_map, double delta,
                                                                   const rtk::TonemapPartial *__restrict__ in,
                                                                   rtk::TonemapPartial *__restrict__ out, double exposure, double auto_key,
                                                                   double *__restrict__ out4) {
    __shared__ double s_t[TM_THREADS];
    __shared__ uint32_t s_c[TM_THREADS];
    const uint32_t tid = threadIdx.x, idx = blockIdx.x * TM_THREADS + tid;
    double t = 0.0;
    uint32_t c = 0;
    if (idx < n_in) {
        if constexpr (First) {
            const double inv = spp_map ? 1.0 / (double)spp_map[idx] : inv_spp;
            const double *v = values + (size_t)idx * 3u;
            t = rtm::rt_log_luminance_term(v[0] * inv, v[1] * inv, v[2] * inv, delta, &c);
        } else {
            t = in[idx].t;
            c = (uint32_t)in[idx].count;
        }
    }
    s_t[tid] = t;
    s_c[tid] = c;
    __syncthreads();
    if (tid < 128) {
        s_t[tid] = s_t[tid] + s_t[tid + 128];
        s_c[tid] = s_c[tid] + s_c[tid + 128];
    }
    __syncthreads();
    if (tid >= 64) return; // one wave64 is left: lanes 0 .. 63 of the block, all of them active below
    t = s_t[tid] + s_t[tid + 64];
    c = s_c[tid] + s_c[tid + 64];
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) { // lane i < stride: e[i] + e[i + stride]; what the other lanes make is never read
        t = t + __shfl_down(t, stride, 64);
        c = c + __shfl_down(c, stride, 64);
    }
    if (tid != 0) return;
    out[blockIdx.x].t = t;
    out[blockIdx.x].count = c;
    if (gridDim.x == 1) rtm::rt_log_average_result(t, c, exposure, auto_key, out4);
}

__device__ __forceinline__ uint8_t tonemap_byte(double sum, double inv, double scale, int32_t op, double w2) {
    const double m = sum * inv;
    const double x = m * scale;
    return rtm::rt_quantise(rtm::rt_gamma_encode(rtm::rt_tonemap(op, x, w2)));
}

// one thread per value: rgb[idx] from values[idx]
__global__ void tonemap_rgb8_kernel(int64_t n_values, const double *__restrict__ values, double inv_spp, const int32_t *__restrict__ spp_map,
                                    double scale, const double *__restrict__ d_scale, int32_t op, double w2, uint8_t *__restrict__ rgb) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_values) return;
    const double inv = spp_map ? 1.0 / (double)spp_map[idx / 3] : inv_spp;
    rgb[idx] = tonemap_byte(values[idx], inv, d_scale ? *d_scale : scale, op, w2);
}

// one thread and one 4-byte store per pixel: red in the low byte, alpha 0xff
__global__ void tonemap_rgba8_kernel(int64_t n_pixels, const double *__restrict__ values, double inv_spp, const int32_t *__restrict__ spp_map,
                                     double scale, const double *__restrict__ d_scale, int32_t op, double w2, uint32_t *__restrict__ rgba) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_pixels) return;
    const double inv = spp_map ? 1.0 / (double)spp_map[idx] : inv_spp;
    const double s = d_scale ? *d_scale : scale;
    rgba[idx] = (uint32_t)tonemap_byte(values[idx * 3 + 0], inv, s, op, w2) | ((uint32_t)tonemap_byte(values[idx * 3 + 1], inv, s, op, w2) << 8) |
                ((uint32_t)tonemap_byte(values[idx * 3 + 2], inv, s, op, w2) << 16) | 0xff000000u;
}

} // namespace

namespace rtk {

void launch_log_average(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double delta, TonemapPartial *partials,
                        double exposure, double auto_key, double *out4, hipStream_t stream) {
    int64_t n = n_pixels, blocks = (n + TM_THREADS - 1) / TM_THREADS;
    hipLaunchKernelGGL(tonemap_level_kernel<true>, dim3((unsigned)blocks), dim3(TM_THREADS), 0, stream, (uint32_t)n, values, inv_spp, spp_map, delta,
                       (const TonemapPartial *)nullptr, partials, exposure, auto_key, out4);
    while (blocks > 1) { // the block results, in block order, are the next level's entries
        const TonemapPartial *in = partials;
        partials += blocks;
        n = blocks;
        blocks = (n + TM_THREADS - 1) / TM_THREADS;
        hipLaunchKernelGGL(tonemap_level_kernel<false>, dim3((unsigned)blocks), dim3(TM_THREADS), 0, stream, (uint32_t)n, (const double *)nullptr, 1.0,
                           (const int32_t *)nullptr, delta, in, partials, exposure, auto_key, out4);
    }
}

void launch_tonemap_rgb8(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale, int32_t op,
                         double w2, uint8_t *rgb, hipStream_t stream) {
    const int64_t n = n_pixels * 3;
    hipLaunchKernelGGL(tonemap_rgb8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, values, inv_spp, spp_map, scale, d_scale, op, w2, rgb);
}

void launch_tonemap_rgba8(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale, int32_t op,
                          double w2, uint8_t *rgba, hipStream_t stream) {
    hipLaunchKernelGGL(tonemap_rgba8_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, n_pixels, values, inv_spp, spp_map, scale,
                       d_scale, op, w2, (uint32_t *)rgba);
}

} // namespace rtk
