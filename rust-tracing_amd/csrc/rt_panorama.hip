// rt_panorama.hip — the cube-to-equirectangular resampler (rt_panorama_device; include/rt_amd.h "panoramas").  Scene-free and its own
// translation unit, as rt_robust.hip, rt_upsample.hip and rt_film.hip are.  The map from an output pixel to its face and taps is shared
// by the pixel's three channels, so the kernel works per PIXEL: thread p owns output pixel p = j * w + i, reads its column's and its
// row's two table entries (neighbouring lanes read neighbouring 16-byte pairs, or one pair when they share a row), and runs
// rt_panorama_shared.h's pixel — the mirror's function.  A tap is a texel's 24 contiguous bytes at a 24-byte stride, loaded as three
// 8-byte values; neighbouring output pixels tap the same or neighbouring texels of one face, so a wave's taps are a few cache lines.
// Every thread stores its own 24 bytes, lanes 24 bytes apart: a wave's three stores together cover 1536 contiguous bytes.  A form that staged a workgroup's 768 values in the LDS and wrote them one value per thread, fully coalesced, was measured
// beside this one and was not faster (DESIGN.md "Panorama"), so it is gone.
// No LDS, no atomics, no scratch, nothing that depends on the launch shape: every value is made by one thread.  Compiled without contraction
// (-ffp-contract=off, no fast-math, IEEE division), like the host mirror.  Indexing is 64-bit.
#include "rt_kernels.h"
#include "rt_panorama_shared.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int PN_THREADS = 256;

__global__ __launch_bounds__(PN_THREADS) void panorama_kernel(int32_t w, int64_t n_pixels, const double *__restrict__ tables,
                                                              const double *__restrict__ faces, int32_t F, int32_t g, double inv_spp,
                                                              double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * PN_THREADS + threadIdx.x;
    if (p >= n_pixels) return;
    const int64_t j = p / w, i = p - j * w;
    const double *col = tables + 2 * i, *row = tables + 2 * (int64_t)w + 2 * j;
    double v[3];
    rtpn::pixel(col[0], col[1], row[0], row[1], faces, F, g, inv_spp, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[p * 3 + k] = v[k];
}

} // namespace

namespace rtk {

void launch_panorama(int32_t w, int32_t h, const double *tables, const double *faces, int32_t face_size, int32_t guard, double inv_spp, double *out,
                     hipStream_t stream) {
    const int64_t n = (int64_t)w * h;   // below 2^27: at most 2^19 workgroups
    hipLaunchKernelGGL(panorama_kernel, dim3((unsigned)((n + PN_THREADS - 1) / PN_THREADS)), dim3(PN_THREADS), 0, stream, w, n, tables, faces, face_size,
                       guard, inv_spp, out);
}

} // namespace rtk
