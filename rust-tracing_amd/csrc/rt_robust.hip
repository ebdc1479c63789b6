// rt_robust.hip — robust frames (rt_robust_device; include/rt_amd.h "robust frames").  Scene-free and its own translation unit, as
// rt_bloom.hip and rt_tonemap.hip are.  The stack is K frames of 3 * w * h doubles, block after block, and the three channels of a
// pixel are combined independently, so the kernel works per VALUE: thread idx owns value idx of every block.  Lane l of a wave reads
// consecutive doubles of block k (one 512-byte run per wave and block, fully coalesced); a thread's K loads are 3wh * 8 bytes apart
// and independent of each other, so all of them are in flight before the first is used.
//   robust_kernel<KMAX, M2>   KMAX = 4, 8, 16, 32 slots for any K <= KMAX; M2: the second output too.  The body is
//                             rt_robust_shared.h's combine<KMAX>: a bitonic network and predicated in-order sums over constant indices,
//                             so the K values never leave the registers (2 KMAX VGPRs; no scratch, no LDS, no barrier).
// A smaller KMAX than the smallest that fits is impossible and a larger one changes no bit (the slots behind K hold the canonical NaN,
// which sorts behind everything): launch_robust takes any of the four that is >= K.  No atomics, nothing that depends on the launch
// shape.  Compiled without contraction (-ffp-contract=off, no fast-math, IEEE division), like the host mirror.  Indexing is 64-bit.
#include "rt_kernels.h"
#include "rt_robust_shared.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int RB_THREADS = 256;

template <int KMAX, bool M2>
__global__ __launch_bounds__(RB_THREADS) void robust_kernel(int64_t total /* 3 w h */, const double *__restrict__ stack, rtrb::Rule rule,
                                                            double *__restrict__ mean_out, double *__restrict__ m2_out) {
    const int64_t idx = (int64_t)blockIdx.x * RB_THREADS + threadIdx.x;
    if (idx >= total) return;
    double v[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) v[k] = k < rule.blocks ? stack[(int64_t)k * total + idx] : 0.0;
    double m2 = 0.0;
    mean_out[idx] = rtrb::combine<KMAX, M2>(v, rule, &m2);
    if constexpr (M2) m2_out[idx] = m2;
}

template <int KMAX>
void launch(int64_t total, const double *stack, const rtrb::Rule &rule, double *mean_out, double *m2_out, hipStream_t stream) {
    const dim3 grid((unsigned)((total + RB_THREADS - 1) / RB_THREADS));
    if (m2_out) hipLaunchKernelGGL((robust_kernel<KMAX, true>), grid, dim3(RB_THREADS), 0, stream, total, stack, rule, mean_out, m2_out);
    else hipLaunchKernelGGL((robust_kernel<KMAX, false>), grid, dim3(RB_THREADS), 0, stream, total, stack, rule, mean_out, m2_out);
}

} // namespace

namespace rtk {

void launch_robust(int32_t kmax, int64_t total, const double *stack, int32_t blocks, int32_t mode, int32_t trim, double gain, double inv_spp,
                   double *mean_out, double *m2_out, hipStream_t stream) {
    const rtrb::Rule rule{blocks, mode, trim, gain, inv_spp};
    const int32_t fit = rtrb::kmax_for(blocks);
    if (kmax < fit) kmax = fit;   // (a form too small for K cannot run it)
    if (kmax <= 4) launch<4>(total, stack, rule, mean_out, m2_out, stream);
    else if (kmax <= 8) launch<8>(total, stack, rule, mean_out, m2_out, stream);
    else if (kmax <= 16) launch<16>(total, stack, rule, mean_out, m2_out, stream);
    else launch<32>(total, stack, rule, mean_out, m2_out, stream);
}

} // namespace rtk
