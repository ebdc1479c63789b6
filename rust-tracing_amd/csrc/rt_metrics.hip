// rt_metrics.hip — frame metrics of librt_amd (rt_frame_error_device, rt_frame_noise_device; include/rt_amd.h "frame metrics").  Scene-free
// and apart from the render kernels, as rt_tonemap.hip is.  One kernel, templated on the term: it reduces one level of the normative
// tree — 256 entries per block, one per thread, `for stride = 128 .. 1: e[i] = e[i] (+) e[i + stride]` — where an entry is a record of
// a few f64 accumulators (sums and maxima) and an integer count.  Strides 128 and 64 go through the LDS, one plane of 256 doubles per
// accumulator (lane i reads doubles i and i + stride of a plane: consecutive 8-byte words, conflict-free); once a single wave64 is left
// the strides 32 .. 1 are cross-lane moves, lane i taking lane i + stride's record: the same pairs in the same order.  Level 0 makes
// each pixel's entry from the frames — a pixel's three doubles lie 24 bytes apart from the next pixel's and are loaded as three 8-byte
// values, as rt_panorama.hip's taps are —; every block writes its record to the workspace, and the block of a one-block level also
// writes the final values.  No atomics: the order is the header's whatever the launch shape.  Everything is f64, each operation
// rounded on its own (-ffp-contract=off, no fast-math, IEEE division and square root); the arithmetic is rt_metrics_shared.h's, which
// the host mirror compiles too, so device and host bits are identical.
#include "rt_kernels.h"
#include "rt_metrics_shared.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int MT_THREADS = 256; // the tree's block: normative, not a tuning choice

// A term: ACCS accumulators; pixel() makes level 0's entry of pixel idx, combine() is (+), result() the final values.
struct ErrorTerm {
    static constexpr int ACCS = rtm::RT_ERROR_ACCS;
    const double *values, *ref;
    const int32_t *spp_map;
    double inv_spp, inv_ref, eps, peak;
    __device__ __forceinline__ void pixel(size_t idx, double e[ACCS], uint32_t *count) const {
        const double inv = spp_map ? 1.0 / (double)spp_map[idx] : inv_spp;
        const double *v = values + idx * 3u, *q = ref + idx * 3u;
        const double m[3] = {v[0] * inv, v[1] * inv, v[2] * inv}, r[3] = {q[0] * inv_ref, q[1] * inv_ref, q[2] * inv_ref};
        rtm::rt_error_term(m, r, eps, e, count);
    }
    static __device__ __forceinline__ void combine(double a[ACCS], uint32_t *ca, const double b[ACCS], uint32_t cb) { rtm::rt_error_combine(a, ca, b, cb); }
    __device__ __forceinline__ void result(const double e[ACCS], uint32_t count, double *out) const { rtm::rt_error_result(e, count, peak, out); }
};

struct NoiseTerm {
    static constexpr int ACCS = rtm::RT_NOISE_ACCS;
    const double *first, *second;
    const int32_t *spp_map;
    int32_t n;
    bool means;
    double eps;
    __device__ __forceinline__ void pixel(size_t idx, double e[ACCS], uint32_t *count) const {
        const double *a = first + idx * 3u, *b = second + idx * 3u;
        const double f[3] = {a[0], a[1], a[2]}, s[3] = {b[0], b[1], b[2]};
        rtm::rt_noise_term(means, f, s, spp_map ? spp_map[idx] : n, eps, e, count);
    }
    static __device__ __forceinline__ void combine(double a[ACCS], uint32_t *ca, const double b[ACCS], uint32_t cb) { rtm::rt_noise_combine(a, ca, b, cb); }
    __device__ __forceinline__ void result(const double e[ACCS], uint32_t count, double *out) const { rtm::rt_noise_result(e, count, out); }
};

// One level.  First: entry idx is pixel idx's term; otherwise it is record idx of `in`.  n_in entries; the grid is ceil(n_in / 256)
// blocks, the entries beyond n_in are the padding (the neutral entry).  A record in the workspace is rtk::METRICS_ENTRY_DOUBLES 8-byte
// words: the accumulators, then the count as a uint64 in the last word.  `result` is written by block 0 of a one-block grid only.
template <class Term, bool First>
__global__ __launch_bounds__(MT_THREADS) void metrics_level_kernel(uint32_t n_in, Term term, const double *__restrict__ in, double *__restrict__ out,
                                                                   double *__restrict__ result) {
    constexpr int A = Term::ACCS, W = rtk::METRICS_ENTRY_DOUBLES;
    __shared__ double s_e[A][MT_THREADS];
    __shared__ uint32_t s_c[MT_THREADS];
    const uint32_t tid = threadIdx.x;
    const size_t idx = (size_t)blockIdx.x * MT_THREADS + tid;
    double e[A];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < A; ++k) e[k] = 0.0;
    if (idx < n_in) {
        if constexpr (First) {
            term.pixel(idx, e, &c);
        } else {
            const double *rec = in + idx * W;
#pragma unroll
            for (int k = 0; k < A; ++k) e[k] = rec[k];
            c = (uint32_t)rtm::f2u(rec[W - 1]);
        }
    }
#pragma unroll
    for (int k = 0; k < A; ++k) s_e[k][tid] = e[k];
    s_c[tid] = c;
    __syncthreads();
    if (tid < 128) {
        double b[A];
#pragma unroll
        for (int k = 0; k < A; ++k) b[k] = s_e[k][tid + 128];
        Term::combine(e, &c, b, s_c[tid + 128]);
#pragma unroll
        for (int k = 0; k < A; ++k) s_e[k][tid] = e[k];
        s_c[tid] = c;
    }
    __syncthreads();
    if (tid >= 64) return; // one wave64 is left: lanes 0 .. 63 of the block, all of them active below
    {
        double b[A];
#pragma unroll
        for (int k = 0; k < A; ++k) b[k] = s_e[k][tid + 64];
        Term::combine(e, &c, b, s_c[tid + 64]);
    }
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) { // lane i < stride: e[i] (+) e[i + stride]; what the other lanes make is never read
        double b[A];
#pragma unroll
        for (int k = 0; k < A; ++k) b[k] = __shfl_down(e[k], stride, 64);
        const uint32_t cb = __shfl_down(c, stride, 64);
        Term::combine(e, &c, b, cb);
    }
    if (tid != 0) return;
    double *rec = out + (size_t)blockIdx.x * W;
#pragma unroll
    for (int k = 0; k < A; ++k) rec[k] = e[k];
#pragma unroll
    for (int k = A; k < W - 1; ++k) rec[k] = 0.0; // (the words a smaller record does not use: no byte of a record is left as it was)
    rec[W - 1] = rtm::u2f((uint64_t)c);
    if (gridDim.x == 1) term.result(e, c, result);
}

template <class Term>
void launch_levels(int64_t n_pixels, const Term &term, double *partials, double *result, hipStream_t stream) {
    int64_t n = n_pixels, blocks = (n + MT_THREADS - 1) / MT_THREADS;
    hipLaunchKernelGGL((metrics_level_kernel<Term, true>), dim3((unsigned)blocks), dim3(MT_THREADS), 0, stream, (uint32_t)n, term, (const double *)nullptr,
                       partials, result);
    while (blocks > 1) { // the block results, in block order, are the next level's entries
        const double *in = partials;
        partials += blocks * rtk::METRICS_ENTRY_DOUBLES;
        n = blocks;
        blocks = (n + MT_THREADS - 1) / MT_THREADS;
        hipLaunchKernelGGL((metrics_level_kernel<Term, false>), dim3((unsigned)blocks), dim3(MT_THREADS), 0, stream, (uint32_t)n, term, in, partials, result);
    }
}

} // namespace

namespace rtk {

void launch_frame_error(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, const double *ref, double inv_ref, double eps,
                        double peak, double *partials, double *out8, hipStream_t stream) {
    launch_levels(n_pixels, ErrorTerm{values, ref, spp_map, inv_spp, inv_ref, eps, peak}, partials, out8, stream);
}

void launch_frame_noise(int64_t n_pixels, bool means, const double *first, const double *second, int32_t n, const int32_t *spp_map, double eps,
                        double *partials, double *out4, hipStream_t stream) {
    launch_levels(n_pixels, NoiseTerm{first, second, spp_map, n, means, eps}, partials, out4, stream);
}

} // namespace rtk
