// rt_bloom_shared.h — what both libraries need of rt_bloom_params on the host side (include/rt_amd.h "bloom"): the defaults, the struct
// sizes known, the checks in the header's order and the workspace's layout, so that rt_bloom_device (rt_api.cpp) and its host mirror
// rth_bloom (host/capi.cpp) refuse the same things with the same words.  Plain C++, no device code; the arithmetic itself is
// rt_shared_math.h's.
#pragma once
#include "rt_amd.h"

#include <cmath>
#include <cstring>

namespace rtbl {

constexpr int64_t MAX_PIXELS = (int64_t)1 << 27;  // w * h must stay below this
constexpr int32_t MAX_LEVELS = 8;

inline void defaults(rt_bloom_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.levels = 5;
    p.threshold = 1.0;
    p.strength = 0.25;
}
inline bool size_known(uint32_t size) { return size >= 8 && size <= sizeof(rt_bloom_params) && size % 8 == 0; }
// the caller's params over the defaults, as far as its struct goes; false: its struct_size is not one this library knows
inline bool resolve(const rt_bloom_params *params, rt_bloom_params &p) {
    defaults(p);
    if (!params) return true;
    if (!size_known(params->struct_size)) return false;
    memcpy(&p, params, params->struct_size);
    return true;
}
inline bool frame_ok(int32_t w, int32_t h) { return w >= 1 && h >= 1 && (int64_t)w * h < MAX_PIXELS; }
inline bool finite_not_negative(double x) { return x >= 0.0 && std::isfinite(x); }
// the first field of resolved params that the calls refuse, as the message's tail; null: all fine
inline const char *bad_field(const rt_bloom_params &p) {
    if (p.levels < 1 || p.levels > MAX_LEVELS) return "levels must be from 1 to 8";
    if (!finite_not_negative(p.threshold)) return "threshold must be a finite number >= 0";
    if (!finite_not_negative(p.strength)) return "strength must be a finite number >= 0";
    return nullptr;
}
// the workspace: three regions (B, H, A) of 3 doubles per pixel, each rounded up to a multiple of 16 bytes
inline int64_t region_bytes(int32_t w, int32_t h) { return ((int64_t)w * h * 3 * (int64_t)sizeof(double) + 15) & ~(int64_t)15; }
inline int64_t workspace_bytes(int32_t w, int32_t h) { return frame_ok(w, h) ? 3 * region_bytes(w, h) : -1; }
// the checks the device call and the mirror share, in the header's order up to the params (device: the pointers are d_values,
// d_mean_out and d_workspace; the mirror has values and out_mean and no workspace); null: all fine, and p is resolved
inline const char *bad_argument(bool device, int32_t w, int32_t h, const void *values, const void *out, const void *workspace, int32_t spp,
                                const rt_bloom_params *params, rt_bloom_params &p) {
    if (w <= 0 || h <= 0) return "width and height must be positive";
    if ((int64_t)w * h >= MAX_PIXELS) return "width x height must be below 2^27 pixels";
    if (!values) return device ? "d_values is null" : "values is null";
    if (!out) return device ? "d_mean_out is null" : "out_mean is null";
    if (device && !workspace) return "d_workspace is null";
    if (spp < 1) return "spp must be at least 1";
    if (!resolve(params, p)) return "rt_bloom_params.struct_size is not one this library knows";
    return bad_field(p);
}

} // namespace rtbl
