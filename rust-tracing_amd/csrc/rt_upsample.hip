// rt_upsample.hip — guided upsampling (rt_upsample_device; include/rt_amd.h "guided upsampling").  Scene-free and its own translation
// unit, as rt_denoise.hip, rt_tonemap.hip and rt_bloom.hip are.
//   upsample_prepare_kernel   one thread per LOW pixel: its record R (with the valid flag) and, per guide given, the mean of the guide's
//                         full-size means over its F x F block, into the workspace's regions of 4 doubles per low pixel.
//   upsample_kernel<HasA, HasG, Lds>   one thread per FULL-size pixel; a workgroup owns a tile of 32 x 8 full-size pixels.
//                         Lds: the low records the tile's taps can reach — columns i0(x_first) - 1 .. i0(x_last) + 2, at most
//                         ceil(31 / F) + 4 = 20 of them, and likewise at most 8 rows — are staged once into the LDS as ten planes of
//                         doubles (R, valid, a_low, g_low), a record's values 160 doubles apart: neighbouring pixels read the same or
//                         the neighbouring double of a plane — a broadcast or consecutive banks within a tile row; a wave spans two tile rows, whose
//                         records lie 0 or 20 doubles apart, so a two-way conflict between the rows is possible.  Expected to be cheap; no
//                         bank-conflict counter was collected.  12.5 KiB.  Records
//                         outside the low frame are never read (the taps skip them) and are not staged.
//                         !Lds: the direct form, every tap from the regions in global memory, where neighbouring pixels' taps are the
//                         same few cache lines.
//                         Both run rt_upsample_pixel of rt_upsample_shared.h — the mirror's function — so they give the same bits.
// No atomics and nothing that depends on the launch shape: every value is made by one thread.  Indexing is 64-bit; grids whose second
// dimension would pass 65 535 walk the rest in a loop.
#include "rt_kernels.h"
#include "rt_upsample_shared.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int UP_THREADS = 256;
constexpr int TILE_W = 32, TILE_H = 8;                       // full-size pixels per workgroup
constexpr int REC_W = (TILE_W - 1 + 1) / 2 + 4, REC_H = (TILE_H - 1 + 1) / 2 + 4; // F = 2 is the worst case: ceil(31 / 2) + 4 = 20, ceil(7 / 2) + 4 = 8
constexpr int REC_N = REC_W * REC_H;
constexpr unsigned GRID_Y_MAX = 65535u;
static_assert(TILE_W * TILE_H == UP_THREADS, "one thread per pixel of the tile");

__global__ __launch_bounds__(UP_THREADS) void upsample_prepare_kernel(rtk::UpsampleArgs u) {
    const int64_t q = (int64_t)blockIdx.x * UP_THREADS + threadIdx.x;
    if (q >= (int64_t)u.lw * u.lh) return;
    const int32_t I = (int32_t)(q % u.lw), J = (int32_t)(q / u.lw);
    rtm::rt_upsample_prepare(I, J, u.w, u.h, u.factor, u.low, u.inv_spp, u.albedo_sum, u.n_a, u.edge_sum, u.n_e, u.albedo_floor, u.rec_r + q * 4,
                             u.albedo_sum ? u.rec_a + q * 4 : nullptr, u.edge_sum ? u.rec_g + q * 4 : nullptr);
}

// a tile's records in the LDS: plane k of record (I, J) at s[k][(J - j_lo) * REC_W + (I - i_lo)]
struct TileRecords {
    const double (*s)[REC_N];
    int32_t i_lo, j_lo;
    __device__ __forceinline__ int at(int32_t I, int32_t J) const { return (J - j_lo) * REC_W + (I - i_lo); }
    __device__ __forceinline__ bool valid(int32_t I, int32_t J) const { return s[3][at(I, J)] != 0.0; }
    __device__ __forceinline__ double R(int32_t I, int32_t J, int k) const { return s[k][at(I, J)]; }
    __device__ __forceinline__ double A(int32_t I, int32_t J, int k) const { return s[4 + k][at(I, J)]; }
    __device__ __forceinline__ double G(int32_t I, int32_t J, int k) const { return s[7 + k][at(I, J)]; }
};

template <bool HasA, bool HasG, bool Lds>
__global__ __launch_bounds__(UP_THREADS) void upsample_kernel(rtk::UpsampleArgs u) {
    __shared__ double s_rec[Lds ? 10 : 1][Lds ? REC_N : 1];
    const int tid = threadIdx.x;
    const int32_t F = u.factor, F2 = 2 * F;
    const int32_t x0 = (int32_t)blockIdx.x * TILE_W, x = x0 + tid % TILE_W;
    const int32_t x_last = (x0 + TILE_W - 1 < u.w ? x0 + TILE_W - 1 : u.w - 1);
    const int32_t i_lo = rtm::rt_up_floor_div(2 * x0 + 1 - F, F2) - 1, i_hi = rtm::rt_up_floor_div(2 * x_last + 1 - F, F2) + 2;
    const int32_t tiles_y = (u.h + TILE_H - 1) / TILE_H;
    const rtm::UpsampleRegions regions{u.rec_r, u.rec_a, u.rec_g, u.lw};
    for (int32_t ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
        const int32_t y0 = ty * TILE_H, y = y0 + tid / TILE_W;
        const int32_t y_last = (y0 + TILE_H - 1 < u.h ? y0 + TILE_H - 1 : u.h - 1);
        const int32_t j_lo = rtm::rt_up_floor_div(2 * y0 + 1 - F, F2) - 1, j_hi = rtm::rt_up_floor_div(2 * y_last + 1 - F, F2) + 2;
        if constexpr (Lds) {
            const int32_t nw = i_hi - i_lo + 1, n = nw * (j_hi - j_lo + 1); // nw <= REC_W and n <= REC_N (the bounds above)
            for (int32_t e = tid; e < n; e += UP_THREADS) {
                const int32_t I = i_lo + e % nw, J = j_lo + e / nw;
                if (I < 0 || I >= u.lw || J < 0 || J >= u.lh) continue;
                const int64_t q = ((int64_t)J * u.lw + I) * 4;
                const int at = (J - j_lo) * REC_W + (I - i_lo);
#pragma unroll
                for (int k = 0; k < 4; ++k) s_rec[k][at] = u.rec_r[q + k];
                if constexpr (HasA) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) s_rec[4 + k][at] = u.rec_a[q + k];
                }
                if constexpr (HasG) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) s_rec[7 + k][at] = u.rec_g[q + k];
                }
            }
            __syncthreads();
        }
        if (x < u.w && y < u.h) {
            const int64_t p = (int64_t)y * u.w + x;
            double ap[3] = {0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0}, out[3];
            if constexpr (HasA) {
#pragma unroll
                for (int k = 0; k < 3; ++k) ap[k] = u.albedo_sum[p * 3 + k] / u.n_a;
            }
            if constexpr (HasG) {
#pragma unroll
                for (int k = 0; k < 3; ++k) gp[k] = u.edge_sum[p * 3 + k] / u.n_e;
            }
            if constexpr (Lds) {
                const TileRecords tile{s_rec, i_lo, j_lo};
                rtm::rt_upsample_pixel<HasA, HasG>(x, y, F, u.lw, u.lh, ap, gp, u.sigma_albedo, u.sigma_edge, u.albedo_floor, tile, tile, out);
            } else {
                rtm::rt_upsample_pixel<HasA, HasG>(x, y, F, u.lw, u.lh, ap, gp, u.sigma_albedo, u.sigma_edge, u.albedo_floor, regions, regions, out);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) u.out[p * 3 + k] = out[k];
            if (u.rgba) u.rgba[p] = rtm::rt_upsample_rgba8(out);
        }
        if constexpr (Lds) __syncthreads(); // the next tile of this workgroup overwrites the records
    }
}

template <bool HasA, bool HasG>
void launch_form(bool lds, dim3 grid, const rtk::UpsampleArgs &u, hipStream_t stream) {
    if (lds) hipLaunchKernelGGL((upsample_kernel<HasA, HasG, true>), grid, dim3(UP_THREADS), 0, stream, u);
    else hipLaunchKernelGGL((upsample_kernel<HasA, HasG, false>), grid, dim3(UP_THREADS), 0, stream, u);
}

} // namespace

namespace rtk {

void launch_upsample_prepare(const UpsampleArgs &u, hipStream_t stream) {
    const int64_t n = (int64_t)u.lw * u.lh;
    hipLaunchKernelGGL(upsample_prepare_kernel, dim3((unsigned)((n + UP_THREADS - 1) / UP_THREADS)), dim3(UP_THREADS), 0, stream, u);
}

void launch_upsample(const UpsampleArgs &u, bool lds, hipStream_t stream) {
    const int64_t tiles_y = ((int64_t)u.h + TILE_H - 1) / TILE_H;
    const dim3 grid((unsigned)((u.w + TILE_W - 1) / TILE_W), (unsigned)(tiles_y < GRID_Y_MAX ? tiles_y : GRID_Y_MAX));
    if (u.albedo_sum && u.edge_sum) launch_form<true, true>(lds, grid, u, stream);
    else if (u.albedo_sum) launch_form<true, false>(lds, grid, u, stream);
    else if (u.edge_sum) launch_form<false, true>(lds, grid, u, stream);
    else launch_form<false, false>(lds, grid, u, stream);
}

} // namespace rtk
