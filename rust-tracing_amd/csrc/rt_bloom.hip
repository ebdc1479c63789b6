// rt_bloom.hip — bloom in front of the tone mapper (rt_bloom_device; include/rt_amd.h "bloom").  Scene-free and its own translation unit,
// as rt_denoise.hip and rt_tonemap.hip are.  A frame is 3 doubles per pixel, row after row, so a row is 3 * w VALUES and a horizontal
// tap at pixel distance s * d is the value 3 * s * d further on: the blur kernels work per value, consecutive lanes on consecutive
// doubles, and a pixel's channel never has to be known.
//   bloom_bright_kernel   one thread per pixel: B0 from the pixel's means, +0.0 into A.
//   bloom_h_kernel        one thread per value of a row, walking down the rows: H from B at any stride (global taps).
//   bloom_v_kernel<Last>  one thread per value: B_k+1 from H at any stride (a vertical tap is s * 3 * w values away), A += B_k+1; on the
//                         last level out = m + strength * (A / K) instead, m from d_values again — there is no output launch.
//   bloom_fused_kernel<S, Last>   a level at stride S = 1, 2 as ONE launch: a workgroup owns a tile of 64 pixels x 16 rows, thread t
//                         the tile's value column t.  It computes H for the tile's rows and the 2 * S halo rows above and below into
//                         the LDS (rows outside the frame are skipped, as the definition skips them, and never read), a barrier, then
//                         the V pass from the LDS with the same fused tail as bloom_v_kernel.  A column's LDS accesses are 8 bytes
//                         per lane, consecutive lanes on consecutive doubles: no bank conflicts.  LDS: (16 + 4 S) x 192 doubles =
//                         30 / 36 KiB.  It reads the halo of neighbouring tiles, so it writes another buffer than it reads.  A thread
//                         walks its column's 20 - 24 rows one after the other, so the form pays only where the tiles fill the machine
//                         (bloom_fused_tiles; DESIGN.md "Bloom": faster at 1200 x 800, slower at 256 x 256, and slower at S = 4).
// No atomics and nothing that depends on the launch shape: every value is made by one thread from rt_shared_math.h's functions, which
// the host mirror (rth_bloom) runs too, compiled without contraction on both sides (-ffp-contract=off, no fast-math, IEEE division).
// Indexing is 64-bit; grids whose second dimension would pass 65 535 walk the rest in a loop.
#include "rt_kernels.h"
#include "rt_shared_math.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int BL_THREADS = 256;
constexpr int TILE_PX = 64, TILE_X = 3 * TILE_PX, TILE_Y = 16; // the fused tile: 192 value columns (one per thread) x 16 rows
constexpr unsigned GRID_Y_MAX = 65535u;

__global__ void bloom_bright_kernel(int64_t n_pixels, const double *__restrict__ values, double inv_spp, const int32_t *__restrict__ spp_map,
                                    double threshold, double *__restrict__ b0, double *__restrict__ a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_pixels) return;
    const double inv = spp_map ? 1.0 / (double)spp_map[idx] : inv_spp;
    const double *v = values + idx * 3;
    double b[3];
    rtm::rt_bloom_bright(v[0] * inv, v[1] * inv, v[2] * inv, threshold, b);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        b0[idx * 3 + c] = b[c];
        a[idx * 3 + c] = 0.0;
    }
}

// which of a value column's five horizontal taps lie inside the row: bit d of the result for the tap at x + step * (d - 2)
__device__ __forceinline__ uint32_t taps_inside(int64_t x, int64_t step, int64_t end) {
    uint32_t inside = 0;
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const int64_t t = x + step * (d - 2);
        if (t >= 0 && t < end) inside |= 1u << d;
    }
    return inside;
}

// the five taps around p at distance `step`, those outside not read
__device__ __forceinline__ double taps_at(const double *p, int64_t step, uint32_t inside) {
    double v[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) v[d] = (inside >> d) & 1u ? p[step * (d - 2)] : 0.0;
    return rtm::rt_bloom_taps(v, inside);
}

// what a V pass does with a value's new B: A += B, and the level's stores — or, on the last level, the output value alone
template <bool Last>
__device__ __forceinline__ void bloom_tail(int64_t idx, double b_new, double *__restrict__ b_out, double *__restrict__ a, const rtk::BloomOutput &o) {
    const double a_new = a[idx] + b_new;
    if constexpr (Last) {
        const double inv = o.spp_map ? 1.0 / (double)o.spp_map[idx / 3] : o.inv_spp;
        const double m = o.values[idx] * inv;
        o.out[idx] = rtm::rt_bloom_output(m, a_new, o.levels, o.strength);
    } else {
        b_out[idx] = b_new;
        a[idx] = a_new;
    }
}

__global__ __launch_bounds__(BL_THREADS) void bloom_h_kernel(int32_t w, int32_t h, int32_t stride, const double *__restrict__ b_in,
                                                             double *__restrict__ h_out) {
    const int64_t row = 3 * (int64_t)w, x = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (x >= row) return;
    const int64_t step = 3 * (int64_t)stride;
    const uint32_t inside = taps_inside(x, step, row);
    for (int64_t j = blockIdx.y; j < h; j += gridDim.y) h_out[j * row + x] = taps_at(b_in + j * row + x, step, inside);
}

template <bool Last>
__global__ __launch_bounds__(BL_THREADS) void bloom_v_kernel(int64_t total /* 3 w h */, int64_t step /* stride * 3 w */, const double *__restrict__ h_in,
                                                             double *__restrict__ b_out, double *__restrict__ a, rtk::BloomOutput o) {
    const int64_t idx = (int64_t)blockIdx.x * BL_THREADS + threadIdx.x;
    if (idx >= total) return;
    bloom_tail<Last>(idx, taps_at(h_in + idx, step, taps_inside(idx, step, total)), b_out, a, o);
}

template <int S, bool Last>
__global__ __launch_bounds__(TILE_X) void bloom_fused_kernel(int32_t w, int32_t h, const double *__restrict__ b_in, double *__restrict__ b_out,
                                                             double *__restrict__ a, rtk::BloomOutput o) {
    constexpr int HALO = 2 * S, ROWS = TILE_Y + 2 * HALO;
    __shared__ double s_h[ROWS][TILE_X];
    const int tid = threadIdx.x;
    const int64_t row = 3 * (int64_t)w, x = (int64_t)blockIdx.x * TILE_X + tid;
    const bool column = x < row; // (a thread beyond the row only keeps the barriers' company)
    const uint32_t inside = taps_inside(x, 3 * S, row);
    const int32_t tiles_y = (h + TILE_Y - 1) / TILE_Y;
    for (int32_t ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
        const int32_t j0 = ty * TILE_Y;
        if (column) {
#pragma unroll 4
            for (int r = 0; r < ROWS; ++r) { // LDS row r holds H of frame row j0 - HALO + r
                const int64_t j = (int64_t)j0 - HALO + r;
                if (j < 0 || j >= h) continue;
                s_h[r][tid] = taps_at(b_in + j * row + x, 3 * S, inside);
            }
        }
        __syncthreads();
        if (column) {
#pragma unroll 4
            for (int t = 0; t < TILE_Y; ++t) {
                const int64_t j = (int64_t)j0 + t;
                if (j >= h) break;
                uint32_t in = 0;
                double v[5];
#pragma unroll
                for (int d = 0; d < 5; ++d) { // the tap at frame row j + S * (d - 2) is LDS row t + S * d, written above iff it is in the frame
                    const int64_t jj = j + S * (d - 2);
                    const bool ok = jj >= 0 && jj < h;
                    in |= ok ? 1u << d : 0u;
                    v[d] = ok ? s_h[t + S * d][tid] : 0.0;
                }
                bloom_tail<Last>(j * row + x, rtm::rt_bloom_taps(v, in), b_out, a, o);
            }
        }
        __syncthreads(); // the next tile of this workgroup overwrites the LDS rows
    }
}

template <int S>
void launch_fused(bool last, dim3 grid, int32_t w, int32_t h, const double *b_in, double *b_out, double *a, const rtk::BloomOutput &o, hipStream_t stream) {
    if (last) hipLaunchKernelGGL((bloom_fused_kernel<S, true>), grid, dim3(TILE_X), 0, stream, w, h, b_in, b_out, a, o);
    else hipLaunchKernelGGL((bloom_fused_kernel<S, false>), grid, dim3(TILE_X), 0, stream, w, h, b_in, b_out, a, o);
}

} // namespace

namespace rtk {

void launch_bloom_bright(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double threshold, double *b0, double *a,
                         hipStream_t stream) {
    hipLaunchKernelGGL(bloom_bright_kernel, dim3((unsigned)((n_pixels + BL_THREADS - 1) / BL_THREADS)), dim3(BL_THREADS), 0, stream, n_pixels, values,
                       inv_spp, spp_map, threshold, b0, a);
}

int64_t bloom_fused_tiles(int32_t w, int32_t h) { return ((3 * (int64_t)w + TILE_X - 1) / TILE_X) * (((int64_t)h + TILE_Y - 1) / TILE_Y); }

void launch_bloom_level_fused(int32_t w, int32_t h, int32_t stride, const double *b_in, double *b_out, double *a, const BloomOutput *last,
                              hipStream_t stream) {
    const int64_t row = 3 * (int64_t)w, tiles_y = ((int64_t)h + TILE_Y - 1) / TILE_Y;
    const dim3 grid((unsigned)((row + TILE_X - 1) / TILE_X), (unsigned)(tiles_y < GRID_Y_MAX ? tiles_y : GRID_Y_MAX));
    const BloomOutput o = last ? *last : BloomOutput{};
    if (stride == 1) launch_fused<1>(last != nullptr, grid, w, h, b_in, b_out, a, o, stream);
    else launch_fused<2>(last != nullptr, grid, w, h, b_in, b_out, a, o, stream);
}

void launch_bloom_h(int32_t w, int32_t h, int32_t stride, const double *b_in, double *h_out, hipStream_t stream) {
    const int64_t row = 3 * (int64_t)w;
    const dim3 grid((unsigned)((row + BL_THREADS - 1) / BL_THREADS), (unsigned)((unsigned)h < GRID_Y_MAX ? (unsigned)h : GRID_Y_MAX));
    hipLaunchKernelGGL(bloom_h_kernel, grid, dim3(BL_THREADS), 0, stream, w, h, stride, b_in, h_out);
}

void launch_bloom_v(int32_t w, int32_t h, int32_t stride, const double *h_in, double *b_out, double *a, const BloomOutput *last, hipStream_t stream) {
    const int64_t row = 3 * (int64_t)w, total = row * h, step = row * stride;
    const dim3 grid((unsigned)((total + BL_THREADS - 1) / BL_THREADS));
    if (last) hipLaunchKernelGGL(bloom_v_kernel<true>, grid, dim3(BL_THREADS), 0, stream, total, step, h_in, b_out, a, *last);
    else hipLaunchKernelGGL(bloom_v_kernel<false>, grid, dim3(BL_THREADS), 0, stream, total, step, h_in, b_out, a, BloomOutput{});
}

} // namespace rtk
