// rt_api.hpp — internals shared by the host-side translation units of librt_amd (rt_api.cpp, rt_debug.cpp, rt_gather.cpp).
#pragma once
#include "rt_amd.h"
#include "rt_amd_debug.h"
#include "rt_scene_plan.hpp"

#include <hip/hip_runtime_api.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace rtapi {

extern thread_local std::string g_last_error;  // rt_last_error() of the calling thread (rt_scene_plan.cpp fail)
extern thread_local uint32_t g_last_launch[4]; // of the calling thread's last render: render-kernel launches, LDS level, workgroup threads, grid
extern thread_local uint32_t g_last_kernel[8]; // ... and which kernel it ran (rt_debug_last_kernel): features, LDS level, ordered, wide, AUX, job mode, ids_ok, threads
extern thread_local uint32_t g_last_start[4];  // ... and how its queries started (rt_debug_last_start): start stage, the leaf's [prim, end), start_inline as launched
#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t _e = (expr);                                                                                \
        if (_e != hipSuccess)                                                                                  \
            return rtapi::fail(_e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,                  \
                               std::string(#expr) + ": " + hipGetErrorString(_e));                             \
    } while (0)

// Per-launch scratch.  A frame that needs several launches (sample sub-ranges, bounded by the sample buffer) alternates between
// two such sets on two internal streams, so that the next launch's workgroups move in as the current one's drain (its tail)
// instead of waiting behind its per-pixel summation.
struct LaunchScratch {
    double *att_stack = nullptr;   // parked colours (KParams::att_stack): full size only for scenes that park colours
    size_t att_bytes = 0;
    uint32_t *att_ids = nullptr;   // parked material indices beyond the eight a lane keeps in registers (KParams::att_ids)
    size_t att_ids_bytes = 0;
    double *world_slots = nullptr; // [6][n_threads]
    size_t world_bytes = 0;
    double *samples = nullptr; // sample buffer of one launch
    size_t sample_bytes = 0;
    uint32_t *job_counter = nullptr;
};
struct Workspace {
    LaunchScratch half[2];
    hipStream_t aux[2] = {nullptr, nullptr};      // created on first use (all of them or none)
    hipEvent_t ev_start = nullptr, ev_sum[2] = {nullptr, nullptr};
    hipEvent_t ev_done = nullptr;                 // recorded on the caller's stream behind every render's last enqueue: what an
                                                  // eviction waits for (the caller's stream handle itself is never touched again)
    size_t sample_budget = 0;                     // > 0: the sample buffer size an out-of-memory back-off arrived at
    unsigned long long *counters = nullptr;
    ViewRec *views = nullptr;                     // views mode: the call's view records (KParams::views); grows on demand
    size_t views_bytes = 0;
    ViewRec *views_host = nullptr;                // pinned staging copy of the same size: what the upload reads after the call returns
    hipEvent_t ev_views = nullptr;                // recorded behind that upload: the next call waits for it before it rewrites views_host
};
void free_workspace(Workspace &w);
// One per (scene, stream).  rt_scene::mu guards only the table and `in_use`; everything slow — draining the stream before a buffer
// grows, hipFree / hipMalloc, creating the internal streams, the enqueues themselves — happens under the slot's own mutex, so renders
// of one scene on DIFFERENT streams never wait for each other (renders on one stream are ordered anyway).
struct WorkspaceSlot {
    std::mutex mu;
    Workspace w;
    int in_use = 0; // renders that hold this slot (from the table look-up to the end of their enqueues): such a slot is never evicted
};

// The caller's rt_scene_options (any struct_size this library has ever shipped, or null) laid over the defaults: every field at or
// beyond the caller's struct_size is the default; RT_ERR_INVALID_ARGUMENT for a size or a walk nobody knows.  One helper for
// rt_scene_create_ex and the layout hooks of rt_debug.cpp, so that what a test inspects is what a scene gets.
int resolve_scene_options(const rt_scene_options *options, rt_scene_options &out, const char *who);
// Process-wide defaults (RT_* environment variables, rt_debug_set_*): read and written under one mutex; a scene takes its
// copy when it is created (walk, refit, tree options) and every launch takes one (thresholds, LDS use).
Tuning tuning_snapshot();
void tuning_update(void (*fn)(Tuning &, const void *), const void *arg);

// the scratch of adaptive sampling's convergence steps (rt_api.cpp): bytes needed; with `buf`, where the parts lie
size_t adaptive_scratch_layout(uint32_t n_list, char *buf, uint32_t *list[2], AdaptiveScratch *x);

template <class T> struct DeviceArray {
    T *ptr = nullptr;
    size_t bytes = 0;
};

} // namespace rtapi

using namespace rtapi; // (an internal header of three translation units)

struct rt_scene {
    int device = 0;
    int n_cus = 0;
    int blocks_per_cu[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}; // [LDS level][kernel variant: dense, dense counted, list, views]
    rtapi::Layout layout;                               // every scalar scene creation decided (rt_scene_plan.hpp): what the launches read
    rtapi::DeviceArray<uint4> lds_image;               // the LDS-resident copy of nodes / spheres / quads (if they fit)
    rtapi::DeviceArray<Node32> nodes;
    rtapi::DeviceArray<Sphere> spheres;
    rtapi::DeviceArray<Quad> quads;
    rtapi::DeviceArray<Instance> insts;
    rtapi::DeviceArray<Medium> media;
    rtapi::DeviceArray<DMaterial> mats;
    rtapi::DeviceArray<rt_texture> texs;
    rtapi::DeviceArray<rt_perlin> perlins;
    rtapi::DeviceArray<ImageRef> images;
    rtapi::DeviceArray<uint8_t> texels;
    rtapi::DeviceArray<double> lut;
    rtapi::DeviceArray<uint4> oimage;                   // ordered layout: the tables of load_opair (global copy)
    rtapi::DeviceArray<OSeq> oseq;                      // ... and the world frame's sequence
    rtapi::DeviceArray<uint4> aux_image;                // materials | textures | frames | media | Perlin for the AUX kernels (0 bytes: not used)
    rt_scene_stats stats{};
    std::mutex mu;
    std::map<hipStream_t, std::unique_ptr<rtapi::WorkspaceSlot>> workspaces; // one per stream: launches on a stream are ordered
    rt_scene_options options;                    // the caller's per-scene options (rt_scene_create_ex); unset fields: process defaults
    std::mutex host_render_mu;                   // the host-memory render entry points (rt_api.cpp render_staged) on one scene run one at a time
    std::map<std::pair<int32_t, int32_t>, uint32_t *> tile_lists; // rt_render_moments_device: (w, h) -> every pixel in tile order, device memory (under mu)
};

namespace rtapi {
// of the last counted render: per profile slot (rounds, active lanes, cycles)
extern std::mutex g_stage_profile_mu;
extern unsigned long long g_stage_profile[PROF_SLOTS * 3];
extern unsigned long long g_visit_stats[VISIT_STATS]; // ... and its record visits by kind (under the same mutex)
} // namespace rtapi
