// rt_tonemap_shared.h — what both libraries need of rt_tonemap_params on the host side (include/rt_amd.h "tone mapping"): the defaults,
// the struct sizes known, and the checks in the header's order, so that rt_tonemap_device (rt_api.cpp) and its host mirror rth_tonemap
// (host/capi.cpp) refuse the same things with the same words; rt_film_device and rth_film ("film output") take the same params and
// checks, and their formats' sizes are here.  Plain C++, no device code; the arithmetic itself is rt_shared_math.h's.
#pragma once
#include "rt_amd.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace rttm {

constexpr int32_t LEVEL_BLOCK = 256;              // entries per block of the reduction tree (normative)
constexpr int64_t MAX_PIXELS = (int64_t)1 << 27;  // w * h must stay below this

inline void defaults(rt_tonemap_params &p) {
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    p.op = RT_TONEMAP_CLAMP;
    p.exposure = 1.0;
    p.auto_key = 0.0;
    p.delta = 1e-4;
    p.white = std::numeric_limits<double>::infinity();
}
inline bool size_known(uint32_t size) { return size >= 8 && size <= sizeof(rt_tonemap_params) && size % 8 == 0; }
// the caller's params over the defaults, as far as its struct goes; false: its struct_size is not one this library knows
inline bool resolve(const rt_tonemap_params *params, rt_tonemap_params &p) {
    defaults(p);
    if (!params) return true;
    if (!size_known(params->struct_size)) return false;
    memcpy(&p, params, params->struct_size);
    return true;
}
inline bool frame_ok(int32_t w, int32_t h) { return w >= 1 && h >= 1 && (int64_t)w * h < MAX_PIXELS; }
inline bool positive_finite(double x) { return x > 0.0 && std::isfinite(x); }
// the first field of resolved params that the calls refuse, as the message's tail; null: all fine
inline const char *bad_field(const rt_tonemap_params &p) {
    if (p.op < RT_TONEMAP_CLAMP || p.op > RT_TONEMAP_ACES) return "op must be RT_TONEMAP_CLAMP, RT_TONEMAP_REINHARD or RT_TONEMAP_ACES (0..2)";
    if (!positive_finite(p.exposure)) return "exposure must be a finite number > 0";
    if (!positive_finite(p.delta)) return "delta must be a finite number > 0";
    if (!(p.auto_key >= 0.0) || !std::isfinite(p.auto_key)) return "auto_key must be a finite number >= 0";
    if (!(p.white > 0.0)) return "white must be > 0 (+inf allowed)";
    return nullptr;
}
// film output (include/rt_amd.h "film output"): bytes per pixel of a format (0: not a format), the frame's bytes (-1: refused), and the
// alignment the format's stores need of the output
inline int32_t film_pixel_bytes(int32_t format) { return format == RT_FILM_RGBE ? 4 : format == RT_FILM_F32 ? 12 : format == RT_FILM_RGB16 ? 6 : 0; }
inline int64_t film_bytes(int32_t w, int32_t h, int32_t format) {
    return frame_ok(w, h) && film_pixel_bytes(format) ? (int64_t)w * h * film_pixel_bytes(format) : -1;
}
inline uintptr_t film_alignment(int32_t format) { return format == RT_FILM_RGB16 ? 2u : 4u; }
// blocks of the level that reduces n entries
inline int64_t level_blocks(int64_t n) { return (n + LEVEL_BLOCK - 1) / LEVEL_BLOCK; }
// the workspace: four doubles of results, then 16 bytes (T, count) per block of every level, level 0 first
inline int64_t workspace_bytes(int32_t w, int32_t h) {
    if (!frame_ok(w, h)) return -1;
    int64_t entries = 0;
    for (int64_t n = (int64_t)w * h;;) {
        n = level_blocks(n);
        entries += n;
        if (n == 1) break;
    }
    return 4 * (int64_t)sizeof(double) + entries * 16;
}

} // namespace rttm
