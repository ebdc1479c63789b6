// rt_robust_shared.h — robust frames (include/rt_amd.h "robust frames"), the text both sides of the boundary compile:
//   rtrb::combine<KMAX>   the per-value body: K block values in, the trimmed mean of their sorted order (and its winsorised M2) out.
//                         The kernel (rt_robust.hip, one thread per value) and the host mirror (rth_robust, host/capi.cpp) run it word
//                         for word, without contraction on either side, so the mirror holds the device's bits.
//   the host-side part    rt_robust_params' defaults, the struct sizes known and the checks in the header's order, so that
//                         rt_robust_device (rt_api.cpp) and rth_robust refuse the same things with the same words.
// combine<KMAX> serves any K <= KMAX (KMAX = 4, 8, 16, 32).  Every array index in it is a compile-time constant once its loops are
// unrolled, so on the device the values stay in registers: the order is a bitonic network of compare-exchanges over KMAX slots, the
// slots behind K filled with the canonical NaN, which sorts last and is bit-identical to every NaN of the input (the definition replaces
// those by it), so the first K slots of the sorted network ARE the K values in order whichever KMAX ran.  What depends on K and t at run
// time is a predicate on the constant index i, never an address.
#pragma once
#include "rt_amd.h"
#include "rt_shared_math.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#include <cstring>
#endif

// (full unrolling is what keeps the device's values in registers; the host's compiler needs no such word)
#if defined(__clang__)
#define RT_ROBUST_UNROLL _Pragma("unroll")
#else
#define RT_ROBUST_UNROLL
#endif

namespace rtrb {

constexpr uint64_t CANONICAL_NAN = 0x7ff8000000000000ull;

struct Rule {
    int32_t blocks;  // K, 1..RT_ROBUST_MAX_BLOCKS
    int32_t mode;    // RT_ROBUST_*
    int32_t trim;    // RT_ROBUST_TRIM's count, >= 0
    double gain;     // RT_ROBUST_GINI's factor
    double inv_spp;  // 1.0 / (double)spp
};

RT_HD bool is_finite(double x) { return ((rtm::f2u(x) >> 52) & 0x7ffu) != 0x7ffu; }
RT_HD double canonical(double x) { return x != x ? rtm::u2f(CANONICAL_NAN) : x; }

// a before b in the total order unless b < a or a alone is a NaN (all NaNs are one bit pattern here: swapping two of them is no change)
RT_HD void order(double &a, double &b) {
    const bool swap = b < a || a != a;
    const double lo = swap ? b : a, hi = swap ? a : b;
    a = lo;
    b = hi;
}

// s[0 .. KMAX-1]: block k's stored value for k < r.blocks (the rest is not read).  Returns `out`; *m2 gets M2 when want_m2.
template <int KMAX, bool WANT_M2>
RT_HD double combine(const double (&stored)[KMAX], const Rule &r, double *m2) {
    const int32_t K = r.blocks;
    double s[KMAX];
RT_ROBUST_UNROLL
    for (int i = 0; i < KMAX; ++i) s[i] = i < K ? canonical(stored[i] * r.inv_spp) : rtm::u2f(CANONICAL_NAN);
    // Order: the bitonic network on KMAX slots, ascending
RT_ROBUST_UNROLL
    for (int k = 2; k <= KMAX; k *= 2) {
RT_ROBUST_UNROLL
        for (int j = k / 2; j > 0; j /= 2) {
RT_ROBUST_UNROLL
            for (int i = 0; i < KMAX; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    if ((i & k) == 0) order(s[i], s[l]);
                    else order(s[l], s[i]);
                }
            }
        }
    }
    // Trim count
    const int32_t tmax = (K - 1) / 2;
    int32_t t = 0;
    if (r.mode == RT_ROBUST_TRIM) t = r.trim < tmax ? r.trim : tmax;
    else if (r.mode == RT_ROBUST_MEDIAN) t = tmax;
    else if (r.mode == RT_ROBUST_GINI) {
        bool finite = true;
        double S = 0.0, W = 0.0;
RT_ROBUST_UNROLL
        for (int i = 0; i < KMAX; ++i) {
            if (i < K) {
                finite = finite && is_finite(s[i]);
                S = S + s[i];
                W = W + (double)(2 * i - K + 1) * s[i];
            }
        }
        if (!finite) t = tmax;
        else if (S > 0.0 && W > 0.0) {
            const double g = (r.gain * (W / S)) * 0.5;
            t = g < (double)tmax ? (int32_t)g : tmax;   // (a g that is no number, or not below tmax, is tmax)
        }
    }
    // Output: the mean of s[t .. K-1-t]
    const int32_t last = K - 1 - t;
    double acc = 0.0, lo = 0.0, hi = 0.0;
RT_ROBUST_UNROLL
    for (int i = 0; i < KMAX; ++i) {
        if (i >= t && i <= last) acc = acc + s[i];
        if (i == t) lo = s[i];
        if (i == last) hi = s[i];
    }
    // (kept values that are all equal are their own mean: no sum of m of them, which need not divide back)
    const double out = lo == hi ? lo + 0.0 : canonical(acc / (double)(K - 2 * t));
    if constexpr (WANT_M2) {
        double q = 0.0;
RT_ROBUST_UNROLL
        for (int i = 0; i < KMAX; ++i) {
            if (i < K) {
                const double w = i < t ? lo : i > last ? hi : s[i];
                const double d = w - out;
                q = q + d * d;
            }
        }
        *m2 = canonical(q);
    }
    return out;
}

// the smallest of the body's four sizes that holds K blocks
RT_HD int32_t kmax_for(int32_t blocks) { return blocks <= 4 ? 4 : blocks <= 8 ? 8 : blocks <= 16 ? 16 : 32; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side: rt_robust_params ----

constexpr int64_t MAX_PIXELS = (int64_t)1 << 27;  // w * h must stay below this
constexpr double DEFAULT_GAIN = 1.0;              // t = floor(G * K / 2): the median from G = 1 - 1/K on (DESIGN.md "Robust frames")

inline void defaults(rt_robust_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.mode = RT_ROBUST_GINI;
    p.trim = 1;
    p.gain = DEFAULT_GAIN;
}
inline bool size_known(uint32_t size) { return size >= 8 && size <= sizeof(rt_robust_params) && size % 8 == 0; }
// the caller's params over the defaults, as far as its struct goes; false: its struct_size is not one this library knows
inline bool resolve(const rt_robust_params *params, rt_robust_params &p) {
    defaults(p);
    if (!params) return true;
    if (!size_known(params->struct_size)) return false;
    memcpy(&p, params, params->struct_size);
    return true;
}
// the first field of resolved params that the calls refuse, as the message's tail; null: all fine
inline const char *bad_field(const rt_robust_params &p) {
    if (p.mode < RT_ROBUST_MEAN || p.mode > RT_ROBUST_GINI) return "mode must be RT_ROBUST_MEAN, RT_ROBUST_TRIM, RT_ROBUST_MEDIAN or RT_ROBUST_GINI (0..3)";
    if (p.trim < 0) return "trim must not be negative";
    if (!(p.gain > 0.0) || !std::isfinite(p.gain)) return "gain must be a finite number > 0";
    return nullptr;
}
// the checks the device call and the mirror share, in the header's order up to the params (device: d_stack, d_mean_out; the mirror:
// stack, out_mean); null: all fine, and p is resolved
inline const char *bad_argument(bool device, int32_t w, int32_t h, int32_t blocks, const void *stack, const void *out, int32_t spp,
                                const rt_robust_params *params, rt_robust_params &p) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (blocks < 1 || blocks > RT_ROBUST_MAX_BLOCKS) return "blocks must be from 1 to 32";
    if (!stack) return device ? "d_stack is null" : "stack is null";
    if (!out) return device ? "d_mean_out is null" : "out_mean is null";
    if (spp < 1) return "spp must be at least 1";
    if (!resolve(params, p)) return "rt_robust_params.struct_size is not one this library knows";
    return bad_field(p);
}
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}
// the overlap refusals, after the params: an output over the stack's `blocks` frames, or the two outputs over each other
inline const char *bad_overlap(bool device, int32_t w, int32_t h, int32_t blocks, const void *stack, const void *out, const void *m2) {
    const size_t frame = (size_t)w * (size_t)h * 3u * sizeof(double);
    if (ranges_overlap(out, frame, stack, frame * (size_t)blocks)) return device ? "d_mean_out must not overlap d_stack" : "out_mean must not overlap stack";
    if (m2 && ranges_overlap(m2, frame, stack, frame * (size_t)blocks)) return device ? "d_m2_out must not overlap d_stack" : "out_m2 must not overlap stack";
    if (m2 && ranges_overlap(m2, frame, out, frame)) return device ? "d_m2_out must not overlap d_mean_out" : "out_m2 must not overlap out_mean";
    return nullptr;
}
inline Rule rule_of(const rt_robust_params &p, int32_t blocks, int32_t spp) { return Rule{blocks, p.mode, p.trim, p.gain, 1.0 / (double)spp}; }

// one value on the host: block k's stored value is stack[k * stride]
template <int KMAX>
inline double combine_strided(const double *stack, size_t stride, const Rule &r, double *m2) {
    double v[KMAX];
    for (int k = 0; k < KMAX; ++k) v[k] = k < r.blocks ? stack[(size_t)k * stride] : 0.0;
    return m2 ? combine<KMAX, true>(v, r, m2) : combine<KMAX, false>(v, r, nullptr);
}
#endif

} // namespace rtrb
