// rt_film.hip — the film output stage of librt_amd (rt_film_device; include/rt_amd.h "film output"): the tone-mapping stage's value
// y = rt_tonemap(op, m * scale, w2), encoded for a file instead of quantised to eight bits.  Scene-free and apart from the render
// kernels, as rt_tonemap.hip is; auto-exposure is that file's reduction (launch_log_average), and the kernels here read its scale from
// the workspace as the tone-mapping value kernels do.  Elementwise and memory-bound: 24 bytes read per pixel, 4, 12 or 6 written.
//   RGBE   one thread per pixel — the shared exponent needs all three channels — and one packed 32-bit store
//   F32    one thread per value, one 32-bit store of the rounded value's bits
//   RGB16  one thread per value, one 16-bit store
// No LDS, no atomics, no scratch.  The encoders are rt_shared_math.h's, which the host mirror (rth_film) runs too.
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ double film_value(double sum, double inv, double scale, int32_t op, double w2) {
    const double m = sum * inv;
    const double x = m * scale;
    return rtm::rt_tonemap(op, x, w2);
}

__global__ void film_rgbe_kernel(int64_t n_pixels, const double *__restrict__ values, double inv_spp, const int32_t *__restrict__ spp_map,
                                 double scale, const double *__restrict__ d_scale, int32_t op, double w2, uint32_t *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_pixels) return;
    const double inv = spp_map ? 1.0 / (double)spp_map[idx] : inv_spp;
    const double s = d_scale ? *d_scale : scale;
    out[idx] = rtm::rt_rgbe_pack(film_value(values[idx * 3 + 0], inv, s, op, w2), film_value(values[idx * 3 + 1], inv, s, op, w2),
                                 film_value(values[idx * 3 + 2], inv, s, op, w2));
}

// one thread per value: Out is uint32_t (the f32's bits) or uint16_t
template <typename Out>
__global__ void film_value_kernel(int64_t n_values, const double *__restrict__ values, double inv_spp, const int32_t *__restrict__ spp_map,
                                  double scale, const double *__restrict__ d_scale, int32_t op, double w2, Out *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_values) return;
    const double inv = spp_map ? 1.0 / (double)spp_map[idx / 3] : inv_spp;
    const double y = film_value(values[idx], inv, d_scale ? *d_scale : scale, op, w2);
    if constexpr (sizeof(Out) == 4) out[idx] = rtm::rt_f32_of(y);
    else out[idx] = rtm::rt_quantise16(rtm::rt_gamma_encode(y));
}

} // namespace

namespace rtk {

void launch_film(int32_t format, int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale,
                 int32_t op, double w2, void *out, hipStream_t stream) {
    const int64_t n = format == RT_FILM_RGBE ? n_pixels : n_pixels * 3;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (format == RT_FILM_RGBE)
        hipLaunchKernelGGL(film_rgbe_kernel, grid, block, 0, stream, n, values, inv_spp, spp_map, scale, d_scale, op, w2, (uint32_t *)out);
    else if (format == RT_FILM_F32)
        hipLaunchKernelGGL(film_value_kernel<uint32_t>, grid, block, 0, stream, n, values, inv_spp, spp_map, scale, d_scale, op, w2, (uint32_t *)out);
    else
        hipLaunchKernelGGL(film_value_kernel<uint16_t>, grid, block, 0, stream, n, values, inv_spp, spp_map, scale, d_scale, op, w2, (uint16_t *)out);
}

} // namespace rtk
