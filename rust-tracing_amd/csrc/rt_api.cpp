// rt_api.cpp — the host side of librt_amd: the C ABI of include/rt_amd.h (scene upload, render launches, frame-end
// helpers).  Plain C++ over the HIP runtime API; the kernels live in rt_kernel.hip and are reached through rt_kernels.h.
#include "rt_api.hpp"
#include "rt_qfilt.hpp"
#include "rt_tonemap_shared.h"
#include "rt_bloom_shared.h"
#include "rt_robust_shared.h"
#include "rt_panorama_shared.h"
#include "rt_metrics_shared.h"
#include "rt_upsample_shared.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <type_traits>

using namespace rtapi;

namespace rtapi {

thread_local uint32_t g_last_launch[4] = {0, 0, 0, 0};
thread_local uint32_t g_last_kernel[8] = {0, 0, 0, 0, 0, 0, 0, 0};
thread_local uint32_t g_last_start[4] = {0, 0, 0, 0};
std::mutex g_stage_profile_mu;
unsigned long long g_stage_profile[PROF_SLOTS * 3] = {0};
unsigned long long g_visit_stats[VISIT_STATS] = {0};

namespace {
std::mutex g_tuning_mu;
Tuning &tuning_locked() { static Tuning t; return t; } // call with g_tuning_mu held
} // namespace
Tuning tuning_snapshot() {
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    return tuning_locked();
}
void tuning_update(void (*fn)(Tuning &, const void *), const void *arg) {
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    fn(tuning_locked(), arg);
}

} // namespace rtapi

namespace {

uint64_t host_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

template <class T> int upload(DeviceArray<T> &dst, const std::vector<T> &src) {
    dst.bytes = src.size() * sizeof(T);
    // never hand the kernel a null table: allocate at least one element
    const size_t alloc = dst.bytes ? dst.bytes : sizeof(T);
    HIP_TRY(hipMalloc((void **)&dst.ptr, alloc));
    if (dst.bytes) HIP_TRY(hipMemcpy(dst.ptr, src.data(), dst.bytes, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(dst.ptr, 0, alloc));
    return RT_OK;
}

} // namespace

namespace rtapi {
void free_workspace(Workspace &w) {
    for (int h = 0; h < 2; ++h) {
        (void)hipFree(w.half[h].att_stack); (void)hipFree(w.half[h].att_ids); (void)hipFree(w.half[h].samples); (void)hipFree(w.half[h].world_slots); (void)hipFree(w.half[h].job_counter);
        if (w.aux[h]) (void)hipStreamDestroy(w.aux[h]);
        if (w.ev_sum[h]) (void)hipEventDestroy(w.ev_sum[h]);
    }
    if (w.ev_start) (void)hipEventDestroy(w.ev_start);
    if (w.ev_done) (void)hipEventDestroy(w.ev_done);
    (void)hipFree(w.counters);
    (void)hipFree(w.views);
    if (w.views_host) (void)hipHostFree(w.views_host);
    if (w.ev_views) (void)hipEventDestroy(w.ev_views);
    w = Workspace();
}
} // namespace rtapi

namespace {

void free_scene(rt_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (auto &kv : s->workspaces) free_workspace(kv.second->w);
    for (auto &kv : s->tile_lists) (void)hipFree(kv.second);
    (void)hipFree(s->nodes.ptr); (void)hipFree(s->spheres.ptr); (void)hipFree(s->quads.ptr); (void)hipFree(s->insts.ptr);
    (void)hipFree(s->media.ptr); (void)hipFree(s->mats.ptr); (void)hipFree(s->texs.ptr); (void)hipFree(s->perlins.ptr);
    (void)hipFree(s->images.ptr); (void)hipFree(s->texels.ptr); (void)hipFree(s->lut.ptr); (void)hipFree(s->lds_image.ptr); (void)hipFree(s->oimage.ptr); (void)hipFree(s->oseq.ptr); (void)hipFree(s->aux_image.ptr);
    delete s;
}

int64_t tiles_total(int32_t w, int32_t h) {
    return (int64_t)((w + RT_TILE_W - 1) / RT_TILE_W) * ((h + RT_TILE_H - 1) / RT_TILE_H);
}
int64_t tiles_local(int32_t w, int32_t h, int32_t shard_index, int32_t shard_count) {
    return (tiles_total(w, h) - shard_index + shard_count - 1) / shard_count;
}
// every pixel of the shard's tiles that lies inside the frame: fn(where its three values start in the shard's tile buffer, where in the frame)
template <class Fn> void for_each_shard_pixel(int32_t w, int32_t h, int32_t shard_index, int32_t shard_count, Fn &&fn) {
    const int32_t tiles_x = (w + RT_TILE_W - 1) / RT_TILE_W;
    const int64_t n_local = tiles_local(w, h, shard_index, shard_count);
    for (int64_t lt = 0; lt < n_local; ++lt) {
        const int64_t k = lt * shard_count + shard_index;
        const int32_t x0 = (int32_t)(k % tiles_x) * RT_TILE_W, y0 = (int32_t)(k / tiles_x) * RT_TILE_H;
        for (int32_t ty = 0; ty < RT_TILE_H; ++ty)
            for (int32_t tx = 0; tx < RT_TILE_W; ++tx) {
                const int32_t i = x0 + tx, j = y0 + ty;
                if (i >= w || j >= h) continue;
                fn((size_t)((lt * RT_TILE_H + ty) * RT_TILE_W + tx) * 3u, ((size_t)j * w + i) * 3u);
            }
    }
}

// One buffer of a host-memory render entry point.  `host` null with bytes > 0: device-only scratch.  bytes 0: no such buffer.
struct HostPart {
    void *host;
    size_t bytes;
    bool upload; // the call continues the caller's running values: copy them to the device before the render
};

// The staging of every host-memory render entry point, past its checks: the scene's device, one allocation for all parts (each starts
// 16-byte aligned; an empty part's device pointer is null), the uploads, `render(d)` with the parts' device pointers on the null stream,
// the downloads of the parts that have a host pointer, in list order.  `serial`: calls on one scene run one at a time (host_render_mu).
// A call that fails behind the allocation may still have launches in flight on the null stream — launch_render's own guard waits for
// its internal streams only — so the device is drained before the buffer is freed, and the sticky error cleared after it.  (rt_render
// and rt_render_views used to free at once.)
template <size_t N, class Render> int render_staged(const char *who, rt_scene *s, bool serial, const HostPart (&parts)[N], Render &&render) {
    std::unique_lock<std::mutex> lock(s->host_render_mu, std::defer_lock);
    if (serial) lock.lock();
    HIP_TRY(hipSetDevice(s->device));
    size_t total = 0;
    for (const HostPart &p : parts) total += align16(p.bytes);
    char *buf = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, total));
    void *d[N];
    for (size_t i = 0, off = 0; i < N; off += align16(parts[i].bytes), ++i) d[i] = parts[i].bytes ? buf + off : nullptr;
    int rc = RT_OK;
    for (size_t i = 0; i < N && rc == RT_OK; ++i)
        if (parts[i].upload && parts[i].host && parts[i].bytes && hipMemcpy(d[i], parts[i].host, parts[i].bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(RT_ERR_HIP, std::string(who) + ": upload of the running values failed");
    if (rc == RT_OK) rc = render(d);
    for (size_t i = 0; i < N && rc == RT_OK; ++i) {
        if (!parts[i].host || !parts[i].bytes) continue;
        const hipError_t e = hipMemcpy(parts[i].host, d[i], parts[i].bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    if (rc != RT_OK) (void)hipDeviceSynchronize();
    (void)hipFree(buf);
    if (rc != RT_OK) (void)hipGetLastError();
    return rc;
}

int normalise_params(const rt_camera *cam, rt_render_params &p) {
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: empty image");
    if ((int64_t)cam->image_width * cam->image_height > 0x7fffffffll)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: image has more than 2^31 pixels");
    if (p.sample_end <= 0) p.sample_end = cam->samples_per_pixel;
    if (p.max_depth <= 0) p.max_depth = cam->max_depth;
    if (p.shard_count <= 0) p.shard_count = 1;
    if (p.sample_begin < 0 || p.sample_end < p.sample_begin) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: bad sample range");
    if (p.shard_index < 0 || p.shard_index >= p.shard_count) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: shard_index out of range");
    if (p.out_layout != RT_OUT_FRAME && p.out_layout != RT_OUT_TILES) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: unknown out_layout");
    if (p.max_depth <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: max_depth must be positive");
    return RT_OK;
}

// the process defaults of this moment with the scene's own options (rt_scene_create_ex) on top
Tuning effective_tuning(const rt_scene *scene) {
    Tuning tn = tuning_snapshot();
    const rt_scene_options &o = scene->options;
    if (o.use_lds >= 0) tn.use_lds = o.use_lds;
    const int32_t th[5] = {o.th_prim, o.th_other, o.th_shade, o.th_box, o.th_new};
    for (int k = 0; k < 5; ++k)
        if (th[k] >= 0 && tn.forced[k] < 0) tn.forced[k] = th[k];
    if (o.sample_buffer_bytes > 0) tn.sample_buffer_bytes = (size_t)o.sample_buffer_bytes;
    if (o.start_shortcut >= 0) tn.start_shortcut = o.start_shortcut;
    if (o.defer_instances >= 0) tn.defer = o.defer_instances;
    if (o.seq_lookahead >= 0) tn.seq_lookahead = o.seq_lookahead;
    if (o.slow_min >= 1) tn.slow_min = o.slow_min;
    if (o.slow_age >= 0) tn.slow_age = o.slow_age;
    if (o.quad_filter >= 0) tn.quad_filter = o.quad_filter;
    if (o.medium_first >= 0) tn.medium_first = o.medium_first;
    return tn;
}

constexpr size_t MAX_WORKSPACES = 4; // per scene: one per stream in use; beyond that the idle ones are released

// List mode (rt_render_pixels_device): the render's "local tiles" are groups of 64 entries of a pixel list, and the sums (and,
// optionally, the sums of squares) go to the listed pixels of a frame.  Everything else — chunks, pipelining, scratch, grid — is
// the dense render's, with n_local = the number of groups.
// a launch's jobs: the job index has 32 bits, and half of them stay free for the grabs past the end
constexpr int64_t MAX_JOBS_PER_LAUNCH = (int64_t)1 << 31;

struct PixelList {
    const uint32_t *pixels;
    int64_t n;
    double *d_sum_sq; // or null
};

// Views mode (rt_render_views_device): the render's "local tiles" are the tiles of view 0's frame, then view 1's, ...; `camera` is
// view 0's (what the views share: frame size, and the defaults of the sample range and the depth); the sums go to one frame per view.
// The records are copied to the workspace per call.  Everything else is the dense render's, with n_local = views x tiles of a frame.
struct ViewTable {
    const ViewRec *recs; // host
    int64_t n;
    double *d_sum_sq = nullptr; // rt_render_views_moments_device: one frame of sums of squares per view beside the sums, or null
};

// Live refinement (rt_render_mean_device): the dense render with `d_out` a frame of running means.  Each launch's samples go into it
// through the reduction's mean fold instead of its sum (rt_kernels.h Reduce); the last launch of the call also writes the display
// frame.  Everything else — chunks, pipelining, scratch, grid — is the dense render's.  With `d_m2` (rt_render_mean_moments_device) the
// fold keeps Welford's M2 in that frame beside the mean.
struct MeanOut {
    uint8_t *d_rgba8; // or null
    double *d_m2;     // or null
};

// The scene-constant part of a launch's parameters at LDS level `lds` under `tn`: the tables, where the regions of the dynamic LDS start
// (rt_scene_plan.hpp), where a query starts.  The per-call and per-launch words are launch_render's.
int scene_params(KParams &K, const rt_scene *scene, int lds, const Tuning &tn) {
    const Layout &L = scene->layout;
    K.nodes = scene->nodes.ptr; K.spheres = scene->spheres.ptr; K.quads = scene->quads.ptr; K.insts = scene->insts.ptr;
    K.media = scene->media.ptr; K.mats = scene->mats.ptr; K.texs = scene->texs.ptr; K.perlins = scene->perlins.ptr;
    K.images = scene->images.ptr; K.texels = scene->texels.ptr; K.srgb_lut = scene->lut.ptr;
    K.n_nodes = L.n_nodes;
    K.id_one = (uint32_t)(scene->mats.bytes / sizeof(DMaterial)) - 1u;
    K.ids_ok = K.id_one < 0xffffu ? 1u : 0u;
    K.lds_image = scene->lds_image.ptr; K.lds_image_bytes = L.lds.prefix_bytes[lds];
    K.lds_off_node_b = L.lds.off_node_b;
    K.lds_off_spheres = L.lds.off_spheres; K.lds_off_quads = L.lds.off_quads;
    K.lds_off_qfilt = (lds == 3 && tn.quad_filter != 0 && L.lds.off_qfilt != 0) ? L.lds.off_qfilt : 0xffffffffu;
    K.lds_world_off = world_in_lds(L, lds) ? (uint32_t)world_offset(L, lds) : 0xffffffffu;
    K.box_extent = L.box_extent;
    K.seq_lookahead = tn.seq_lookahead ? 1u : 0u;
    K.medium_first = tn.medium_first ? 1u : 0u;
    K.inst_shortcut = tn.start_shortcut ? 1u : 0u;
    K.slow_min = (uint32_t)tn.slow_min; K.slow_age = (uint32_t)tn.slow_age;
    K.o_start_stage = tn.start_shortcut ? L.start.stage : 0u; K.o_start_prim = L.start.prim; K.o_start_end = L.start.end;
    K.o_start_rest = L.start.rest; K.o_start_slot = L.start.slot;
    K.setaside_direct = tn.wide_setaside != 0 ? 1u : 0u;
    // the inline start test (path_kernel): the shortcut's leaf is one sphere (OrderedKind SPHERES = Stage ST_SPHERE = 1)
    K.start_inline = (tn.start_inline != 0 && K.o_start_stage == (uint32_t)OK_SPHERES && K.o_start_end == K.o_start_prim + 1u) ? 1u : 0u;
    if (L.wide) { // the start shortcut's entry as the kernel pushes it (rt_kernel.hip W_SHIFT: 2-byte entries in the LDS kernels)
        // An entry is a record's index and, above it, the mask of its children NOT to be looked at: an inner record set aside as itself is
        // its bare index.  No entry at all is all ones, which no entry is (one with all four children gone is never made).
        const uint32_t w_shift = lds != 0 ? 12u : 26u;
        if (K.setaside_direct && L.start.direct != 0xffffffffu) K.o_start_rest = L.start.direct;
        else if (L.start.rest != 0u) K.o_start_rest = L.o_root | ((~L.start.rest & 0xfu) << w_shift);
        else K.o_start_rest = 0xffffffffu;
        // (no real entry may read as S_EXIT, all ones in the entry's width)
        if (K.o_start_rest != 0xffffffffu && (K.o_start_rest & (lds != 0 ? 0xffffu : 0xffffffffu)) == (lds != 0 ? 0xffffu : 0xffffffffu))
            return fail(RT_ERR_INVALID_ARGUMENT, "start shortcut: entry reads as S_EXIT");
    }
    K.oimage = scene->oimage.ptr; K.o_root = L.o_root; K.oseq = scene->oseq.ptr; K.n_oseq = L.n_oseq; K.lds_stack_off = L.lds.prefix_bytes[lds];
    K.lds_seq_off = (uint32_t)seq_offset(L, lds);
    K.aux_image = scene->aux_image.ptr; K.aux_bytes = L.aux.bytes; K.lds_aux_off = (uint32_t)aux_offset(L, lds);
    K.aux_off_mats = L.aux.off[0]; K.aux_off_texs = L.aux.off[1]; K.aux_off_insts = L.aux.off[2];
    K.aux_off_media = L.aux.off[3]; K.aux_off_perlins = L.aux.off[4];
    K.lds_prof_off = (uint32_t)prof_offset(L, lds);
    // (a lane keeps the instances it has yet to walk as one 32-bit mask of their indices)
    K.defer_instances = (L.ordered && tn.defer != 0 && scene->insts.bytes / sizeof(Instance) <= 32u) ? 1u : 0u;
    return RT_OK;
}

int launch_render(rt_scene *scene, const rt_camera *camera, rt_render_params p, double *d_out, hipStream_t stream,
                  rt_counters *out_counters, const PixelList *list = nullptr, const ViewTable *views = nullptr, const MeanOut *mean = nullptr) {
    int rc = normalise_params(camera, p);
    if (rc != RT_OK) return rc;
    if (list && (p.shard_count != 1 || p.out_layout != RT_OUT_FRAME))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_pixels_device: a pixel list needs shard_count 1 and out_layout RT_OUT_FRAME");
    if (list && (int64_t)camera->image_width * camera->image_height >= ((int64_t)1 << 27))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_pixels_device: a pixel list needs an image of fewer than 2^27 pixels");
    HIP_TRY(hipSetDevice(scene->device));
    const bool counted = out_counters != nullptr;
    const int64_t tiles_per_view = tiles_total(camera->image_width, camera->image_height);
    const int64_t n_local = views ? views->n * tiles_per_view
                                  : list ? (list->n + 63) / 64 : tiles_local(camera->image_width, camera->image_height, p.shard_index, p.shard_count);
    const int64_t n_samples_total = (int64_t)p.sample_end - p.sample_begin;
    if (n_local <= 0 || n_samples_total <= 0) {
        if (out_counters) *out_counters = rt_counters{};
        return RT_OK;
    }
    const Tuning tn = effective_tuning(scene);

    // samples per launch: bounded by the sample buffer and by the 32-bit job index.  A frame that needs more than one launch is
    // pipelined over two scratch sets (half the budget each) unless that is switched off or the kernel is the instrumented one.
    const int64_t bytes_per_sample_row = n_local * 64 * 3 * (int64_t)sizeof(double);
    const int64_t max_by_index = MAX_JOBS_PER_LAUNCH / (n_local * 64);
    auto chunk_for = [&](size_t budget) {
        int64_t c = (int64_t)(budget / (size_t)bytes_per_sample_row);
        if (c > max_by_index) c = max_by_index;
        if (c > n_samples_total) c = n_samples_total;
        return c;
    };
    int64_t chunk = chunk_for(tn.sample_buffer_bytes);
    if (chunk < 1) return fail(RT_ERR_UNSUPPORTED, "rt_render: one sample per pixel does not fit the sample buffer");
    bool pipelined = !counted && tn.overlap != 0 && chunk < n_samples_total && chunk_for(tn.sample_buffer_bytes / 2) >= 1;
    if (pipelined) chunk = chunk_for(tn.sample_buffer_bytes / 2);

    const Layout &L = scene->layout;
    const int lds = tn.use_lds != 0 ? L.lds.level : 0;
    const int threads = block_threads(L, lds);
    const int jobs = views ? JOBS_VIEWS : list ? JOBS_LIST : JOBS_DENSE;
    const int bpc = scene->blocks_per_cu[lds][kernel_variant(counted, jobs)];
    const size_t dyn_lds = dynamic_lds_bytes(L, lds, counted);
    // persistent grid: every resident wave pulls jobs until none are left
    int64_t grid = (int64_t)scene->n_cus * bpc;
    const int64_t waves_per_block = threads / 64;
    // (a small frame gets a smaller grid: a wave with fewer than MIN_JOBS_PER_WAVE jobs costs more to start than it adds)
    const int64_t max_useful = (n_local * 64 * chunk + MIN_JOBS_PER_WAVE * waves_per_block - 1) / (MIN_JOBS_PER_WAVE * waves_per_block);
    if (grid > max_useful) grid = max_useful;
    if (grid < 1) grid = 1;
    const uint32_t n_threads = (uint32_t)(grid * threads);

    // The scratch of this (scene, stream).  Under the scene's lock: the table look-up, the in-use mark, and — a new stream and a full
    // table — taking the idle slots OUT of the table.  Everything that can wait (an evicted slot's last render, a drain before a buffer
    // grows, hipFree / hipMalloc) and the enqueues happen outside it, under the slot's own mutex: renders on other streams go on.
    // Only slots nobody holds are ever evicted, after waiting for the event their last render recorded (a library-owned handle:
    // the caller's stream may be gone by then).
    Workspace ws;
    WorkspaceSlot *slot = nullptr;
    std::vector<std::unique_ptr<WorkspaceSlot>> evicted;
    {
        std::lock_guard<std::mutex> lock(scene->mu);
        if (scene->workspaces.find(stream) == scene->workspaces.end() && scene->workspaces.size() >= MAX_WORKSPACES) {
            // (slots in use stay: the table then grows past its nominal size rather than pull scratch from under a render)
            for (auto it = scene->workspaces.begin(); it != scene->workspaces.end();) {
                if (it->second->in_use != 0) { ++it; continue; }
                evicted.push_back(std::move(it->second));
                it = scene->workspaces.erase(it);
            }
        }
        std::unique_ptr<WorkspaceSlot> &entry = scene->workspaces[stream];
        if (!entry) entry.reset(new WorkspaceSlot());
        slot = entry.get();
        slot->in_use++;
    }
    struct Release { // (declared before the slot's lock: runs after it is dropped)
        rt_scene *scene; WorkspaceSlot *slot; hipStream_t stream;
        bool enqueued = false, completed = false;
        ~Release() {
            // a render that failed after some launches were enqueued: what is in flight is waited for and the slot's event recorded all the
            // same, so that a later eviction never frees scratch a kernel still uses
            if (enqueued && !completed) {
                for (int h = 0; h < 2; ++h) if (slot->w.aux[h]) (void)hipStreamSynchronize(slot->w.aux[h]);
                if (slot->w.ev_done) (void)hipEventRecord(slot->w.ev_done, stream);
                (void)hipGetLastError();
            }
            std::lock_guard<std::mutex> lock(scene->mu);
            if (slot->in_use > 0) slot->in_use--;
        }
    } release{scene, slot, stream};
    for (auto &old : evicted) {
        if (old->w.ev_done) (void)hipEventSynchronize(old->w.ev_done);
        free_workspace(old->w);
    }
    if (!evicted.empty()) (void)hipGetLastError();
    evicted.clear();
    const bool colours = L.parks_colours;
    std::unique_lock<std::mutex> slot_lock(slot->mu); // held to the end of the enqueues
    {
        Workspace &w = slot->w;
        const size_t need_att = colours ? ((size_t)p.max_depth + 1u) * n_threads * 3u * sizeof(double) : sizeof(double); // + a light's emitted colour
        if (need_att / sizeof(double) >= ((size_t)1 << 32)) return fail(RT_ERR_UNSUPPORTED, "rt_render: max_depth too large for the attenuation stack's 32-bit indices");
        const size_t need_ids = ((size_t)p.max_depth + 1u) * n_threads * sizeof(uint32_t);
        if (need_ids / sizeof(uint32_t) >= ((size_t)1 << 32)) return fail(RT_ERR_UNSUPPORTED, "rt_render: max_depth too large for the index stack's 32-bit indices");
        const size_t need_world = (size_t)6 * n_threads * sizeof(double);
        if (!w.ev_done) HIP_TRY(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
        if (pipelined && !w.aux[0]) { // both streams and all three events, or none of them
            hipStream_t st[2] = {nullptr, nullptr};
            hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
            hipError_t e = hipSuccess;
            for (int h = 0; h < 2 && e == hipSuccess; ++h) e = hipStreamCreateWithFlags(&st[h], hipStreamNonBlocking);
            for (int h = 0; h < 3 && e == hipSuccess; ++h) e = hipEventCreateWithFlags(&ev[h], hipEventDisableTiming);
            if (e != hipSuccess) {
                for (int h = 0; h < 2; ++h) if (st[h]) (void)hipStreamDestroy(st[h]);
                for (int h = 0; h < 3; ++h) if (ev[h]) (void)hipEventDestroy(ev[h]);
                return fail(RT_ERR_HIP, std::string("rt_render: internal streams: ") + hipGetErrorString(e));
            }
            w.aux[0] = st[0]; w.aux[1] = st[1]; w.ev_sum[0] = ev[0]; w.ev_sum[1] = ev[1]; w.ev_start = ev[2];
        }
        // (an earlier out-of-memory back-off on this stream is remembered: the buffer it arrived at is the budget from then on)
        if (w.sample_budget > 0) {
            const int64_t c = chunk_for(w.sample_budget);
            if (c >= 1 && c < chunk) chunk = c;
        }
        // (every earlier launch on this stream ends with the stream waiting for the internal ones: draining it drains them)
        bool drained = false;
        auto drain = [&]() -> int { if (!drained) { HIP_TRY(hipStreamSynchronize(stream)); drained = true; } return RT_OK; };
        for (int h = 0; h < (pipelined ? 2 : 1); ++h) {
            LaunchScratch &x = w.half[h];
            if (x.att_bytes < need_att) {
                if ((rc = drain()) != RT_OK) return rc;
                if (x.att_stack) HIP_TRY(hipFree(x.att_stack));
                x.att_stack = nullptr; x.att_bytes = 0;
                HIP_TRY(hipMalloc((void **)&x.att_stack, need_att));
                x.att_bytes = need_att;
            }
            if (x.att_ids_bytes < need_ids) {
                if ((rc = drain()) != RT_OK) return rc;
                if (x.att_ids) HIP_TRY(hipFree(x.att_ids));
                x.att_ids = nullptr; x.att_ids_bytes = 0;
                HIP_TRY(hipMalloc((void **)&x.att_ids, need_ids));
                x.att_ids_bytes = need_ids;
            }
            if (x.world_bytes < need_world) {
                if ((rc = drain()) != RT_OK) return rc;
                if (x.world_slots) HIP_TRY(hipFree(x.world_slots));
                x.world_slots = nullptr; x.world_bytes = 0;
                HIP_TRY(hipMalloc((void **)&x.world_slots, need_world));
                x.world_bytes = need_world;
            }
            size_t need_samples = (size_t)bytes_per_sample_row * (size_t)chunk;
            if (x.sample_bytes < need_samples) {
                if ((rc = drain()) != RT_OK) return rc;
                if (x.samples) HIP_TRY(hipFree(x.samples));
                x.samples = nullptr; x.sample_bytes = 0;
                // a device short of memory gets a smaller chunk (more launches), not an error
                for (;;) {
                    const hipError_t e = hipMalloc((void **)&x.samples, need_samples);
                    if (e == hipSuccess) break;
                    (void)hipGetLastError();
                    x.samples = nullptr;
                    if (e != hipErrorOutOfMemory || chunk <= 1)
                        return fail(e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP, std::string("rt_render: sample buffer: ") + hipGetErrorString(e));
                    chunk = (chunk + 1) / 2;
                    need_samples = (size_t)bytes_per_sample_row * (size_t)chunk;
                    w.sample_budget = need_samples;
                }
                x.sample_bytes = need_samples;
            }
            if (!x.job_counter) HIP_TRY(hipMalloc((void **)&x.job_counter, sizeof(uint32_t)));
        }
        if (!w.counters) HIP_TRY(hipMalloc((void **)&w.counters, COUNTER_WORDS * sizeof(unsigned long long)));
        if (views && w.views_bytes < (size_t)views->n * sizeof(ViewRec)) {
            if ((rc = drain()) != RT_OK) return rc;
            if (w.views) HIP_TRY(hipFree(w.views));
            w.views = nullptr; w.views_bytes = 0;
            if (w.views_host) HIP_TRY(hipHostFree(w.views_host));
            w.views_host = nullptr;
            HIP_TRY(hipMalloc((void **)&w.views, (size_t)views->n * sizeof(ViewRec)));
            HIP_TRY(hipHostMalloc((void **)&w.views_host, (size_t)views->n * sizeof(ViewRec), hipHostMallocDefault));
            w.views_bytes = (size_t)views->n * sizeof(ViewRec);
        }
        if (views) {
            if (!w.ev_views) HIP_TRY(hipEventCreateWithFlags(&w.ev_views, hipEventDisableTiming));
            // the staging copy is the slot's own pinned memory: the call's records go there once the previous call's upload has run
            // (that upload sits ahead of its own render's kernels, so one views render may be in flight while the next is enqueued)
            HIP_TRY(hipEventSynchronize(w.ev_views));
            memcpy(w.views_host, views->recs, (size_t)views->n * sizeof(ViewRec));
        }
        ws = w;
    }
    release.enqueued = true; // (from here on something may be in flight on `stream` or the internal streams)
    if (counted) HIP_TRY(hipMemsetAsync(ws.counters, 0, COUNTER_WORDS * sizeof(unsigned long long), stream));
    // (in stream order behind the previous render's reads of the table; from pinned memory, so a true asynchronous copy)
    if (views) {
        HIP_TRY(hipMemcpyAsync(ws.views, ws.views_host, (size_t)views->n * sizeof(ViewRec), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ws.ev_views, stream));
    }

    KParams K{};
    if ((rc = scene_params(K, scene, lds, tn)) != RT_OK) return rc;
    K.out = d_out;
    K.counters = counted ? ws.counters : nullptr;
    K.cam = *camera;
    K.seed_mixed = host_mix64(p.seed + 0x9E3779B97F4A7C15ull);
    K.n_threads = n_threads;
    K.max_depth = p.max_depth;
    K.shard_index = p.shard_index; K.shard_count = p.shard_count; K.out_layout = p.out_layout;
    K.tiles_x = (camera->image_width + RT_TILE_W - 1) / RT_TILE_W;
    K.inv_tiles_x = 1.0 / (double)K.tiles_x;
    K.n_local_tiles = (uint32_t)n_local;
    if (list) {
        K.pixel_list = list->pixels; K.n_list = (uint32_t)list->n; K.out_sq = list->d_sum_sq;
        K.inv_width = 1.0 / (double)camera->image_width;
    }
    if (mean) K.out_sq = mean->d_m2;
    if (views) {
        K.views = ws.views; K.tiles_per_view = (uint32_t)tiles_per_view; K.inv_tiles_per_view = 1.0 / (double)tiles_per_view;
        K.out_sq = views->d_sum_sq; // (read by Reduce::ViewsMoments only)
    }
    {
        const uint32_t kf = kernel_features_for(L.features, lds, L.ordered);
        const Thresholds th = tn.pick(kf == FEAT_SPHERES_SOLID ? (L.ordered ? tn.spheres_solid : tn.spheres_threaded) : (kf == FEAT_QUADS_FRAMES ? (scene->insts.bytes ? tn.quads_frames : tn.quads_only) : (L.ordered ? (lds == 0 ? tn.ordered_global : tn.ordered_general) : tn.general)));
        K.th_prim = th.prim; K.th_other = th.other; K.th_shade = th.shade; K.th_box = th.box; K.th_new = th.newjob;
        auto byte = [](uint32_t v) { return v > 255u ? 255u : v; };
        K.th_pack = byte(th.prim) | (byte(th.other) << 8) | (byte(th.shade) << 16) | (byte(th.box) << 24);
    }

    // Launch k renders samples [sb, sb + ns) into its scratch set's sample buffer; the route's reduction kernel then folds them into
    // `out` in sample order.  Pipelined: launch k runs on internal stream k % 2; its reduction waits for launch k - 1's (the folds
    // stay in order) while the render kernel of launch k + 1, on the other stream, takes the CUs that launch k's tail frees.
    const Reduce reduce = mean    ? (mean->d_m2 ? Reduce::MeanMoments : Reduce::Mean)
                          : views ? (views->d_sum_sq ? Reduce::ViewsMoments : Reduce::Views)
                          : list  ? Reduce::Listed
                                  : Reduce::Sum;
    if (pipelined) {
        HIP_TRY(hipEventRecord(ws.ev_start, stream));
        for (int h = 0; h < 2; ++h) HIP_TRY(hipStreamWaitEvent(ws.aux[h], ws.ev_start, 0));
    }
    const unsigned sum_grid = (unsigned)((n_local * 64 + 255) / 256);
    int64_t k = 0;
    for (int64_t sb = p.sample_begin; sb < p.sample_end; sb += chunk, ++k) {
        const int64_t ns = (p.sample_end - sb) < chunk ? (p.sample_end - sb) : chunk;
        const int h = pipelined ? (int)(k & 1) : 0;
        const hipStream_t s = pipelined ? ws.aux[h] : stream;
        const LaunchScratch &x = ws.half[h];
        K.samples = x.samples; K.att_stack = x.att_stack; K.att_ids = x.att_ids; K.job_counter = x.job_counter; K.world_slots = x.world_slots;
        K.sample_begin = (int32_t)sb;
        K.n_samples = (uint32_t)ns;
        K.n_jobs = (uint32_t)(n_local * 64 * ns);
        K.inv_n_samples = 1.0 / (double)ns;
        {
            // ~32 grabs per wave or more, rounded down to a multiple of 64 within [MIN, MAX]
            const int64_t waves = grid * waves_per_block;
            int64_t per_grab = (int64_t)K.n_jobs / (waves * 32);
            if (tn.jobs_per_grab > 0) per_grab = tn.jobs_per_grab;
            per_grab = per_grab / 64 * 64;
            if (per_grab > MAX_JOBS_PER_GRAB) per_grab = MAX_JOBS_PER_GRAB;
            if (per_grab < MIN_JOBS_PER_GRAB) per_grab = MIN_JOBS_PER_GRAB;
            K.jobs_per_grab = (uint32_t)per_grab;
            // (RT_GRAB_TAPER=0 switches the taper off: every grab is jobs_per_grab)
            K.grab_taper = tn.grab_taper > 0 ? 1.0f / (float)(waves * tn.grab_taper) : 1.0f; // (default 8, tools/sweep_grabs.sh)
        }
        K.accumulate = (p.accumulate || sb > p.sample_begin) ? 1 : 0;
        HIP_TRY(hipMemsetAsync(x.job_counter, 0, sizeof(uint32_t), s));
        {
            void *args[] = {(void *)&K};
            const uint32_t kf = kernel_features_for(L.features, lds, L.ordered);
            const void *fn = path_kernel_for(lds, counted, kf, L.ordered, aux_in_lds(L, lds), L.wide, jobs);
            HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)grid), dim3(threads), args, dyn_lds, s));
        }
        HIP_TRY(hipGetLastError());
        if (pipelined && k > 0) HIP_TRY(hipStreamWaitEvent(s, ws.ev_sum[h ^ 1], 0));
        if (mean) K.mean_rgba8 = sb + ns >= p.sample_end ? mean->d_rgba8 : nullptr; // (the call's last launch: the frame the caller shows)
        launch_reduce_samples(reduce, K, sum_grid, s);
        HIP_TRY(hipGetLastError());
        if (pipelined) HIP_TRY(hipEventRecord(ws.ev_sum[h], s));
    }
    if (pipelined) HIP_TRY(hipStreamWaitEvent(stream, ws.ev_sum[(k - 1) & 1], 0)); // (the last sum waited for all before it)
    HIP_TRY(hipEventRecord(ws.ev_done, stream));
    release.completed = true;
    g_last_launch[0] = (uint32_t)k; g_last_launch[1] = (uint32_t)lds; g_last_launch[2] = (uint32_t)threads; g_last_launch[3] = (uint32_t)grid;
    g_last_kernel[0] = kernel_features_for(L.features, lds, L.ordered); g_last_kernel[1] = (uint32_t)lds;
    g_last_kernel[2] = L.ordered ? 1u : 0u; g_last_kernel[3] = L.wide ? 1u : 0u; g_last_kernel[4] = aux_in_lds(L, lds) ? 1u : 0u;
    g_last_kernel[5] = (uint32_t)jobs; g_last_kernel[6] = K.ids_ok; g_last_kernel[7] = (uint32_t)threads;
    g_last_start[0] = L.ordered ? K.o_start_stage : 0u; g_last_start[1] = K.o_start_prim; g_last_start[2] = K.o_start_end; g_last_start[3] = L.ordered ? K.start_inline : 0u;

    if (counted) {
        unsigned long long host[COUNTER_WORDS];
        HIP_TRY(hipMemcpyAsync(host, ws.counters, sizeof host, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        {
            std::lock_guard<std::mutex> lock(g_stage_profile_mu);
            for (uint32_t q = 0; q < PROF_SLOTS * 3u; ++q) g_stage_profile[q] = host[10 + q];
            for (uint32_t q = 0; q < VISIT_STATS; ++q) g_visit_stats[q] = host[10 + PROF_SLOTS * 3u + q];
        }
        out_counters->samples = host[0]; out_counters->rays = host[1]; out_counters->node_visits = host[2];
        out_counters->sphere_tests = host[3]; out_counters->quad_tests = host[4]; out_counters->medium_visits = host[5];
        out_counters->rng_draws = host[6]; out_counters->noise_evals = host[7]; out_counters->image_lookups = host[8];
        out_counters->instance_enters = host[9];
    }
    return RT_OK;
}

} // namespace

namespace rtapi {
void adaptive_defaults(rt_adaptive_params &a) {
    memset(&a, 0, sizeof a);
    a.struct_size = (uint32_t)sizeof a;
    a.min_spp = 16; a.batch_spp = 16;
    a.rel_threshold = 0.02; a.abs_threshold = 1e-3;
}

// The adaptive parameters and the render parameters they constrain, checked before the scene handle and the device (a caller finds
// out what is wrong without a GPU).  Fills the effective parameters, the normalised render parameters and max_spp.
int check_adaptive(const rt_camera *camera, const rt_render_params *params, const rt_adaptive_params *adaptive, const char *who,
                   rt_adaptive_params &a, rt_render_params &p, int32_t &max_spp) {
    const std::string w(who);
    if (!adaptive) return fail(RT_ERR_INVALID_ARGUMENT, w + ": adaptive is null");
    const uint32_t size = adaptive->struct_size;
    if (size < 8 || size > sizeof a || size % 4 != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": rt_adaptive_params.struct_size is not one this library knows");
    adaptive_defaults(a);
    memcpy(&a, adaptive, size); // (an older, shorter struct: the fields it lacks keep their defaults)
    a.struct_size = (uint32_t)sizeof a;
    if (a.batch_spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": batch_spp must be at least 1");
    if (!(a.rel_threshold >= 0.0)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": rel_threshold must be a number >= 0");
    if (!(a.abs_threshold >= 0.0)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": abs_threshold must be a number >= 0");
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, w + ": camera is null");
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, w + ": params is null");
    p = *params;
    if (p.shard_count != 1 && p.shard_count > 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": shard_count must be 1 (adaptive sampling renders the whole frame on one device)");
    if (p.sample_begin != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": sample_begin must be 0");
    if (p.accumulate != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": accumulate must be 0");
    if (p.out_layout != RT_OUT_FRAME) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_layout must be RT_OUT_FRAME");
    if (int rc = normalise_params(camera, p)) return rc;
    if ((int64_t)camera->image_width * camera->image_height >= ((int64_t)1 << 27))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": adaptive sampling needs an image of fewer than 2^27 pixels");
    max_spp = p.sample_end;
    if (a.min_spp > max_spp) a.min_spp = max_spp;
    if (max_spp >= 2 && a.min_spp < 2) return fail(RT_ERR_INVALID_ARGUMENT, w + ": min_spp must be at least 2");
    return RT_OK;
}

// The device scratch of the convergence steps over lists of at most n_list entries (a multiple of 64), laid out in one buffer: two
// lists, a ballot per wave of the step, a count per block, the survivor count (16 bytes).  Returns the bytes needed; with a buffer,
// also where each part lies.  render_adaptive and the test hook rt_debug_adaptive_step size and cut their scratch with this.
size_t adaptive_scratch_layout(uint32_t n_list, char *buf, uint32_t *list[2], AdaptiveScratch *x) {
    const uint32_t blocks = (n_list + 255u) / 256u;
    const size_t list_bytes = align16((size_t)n_list * 4u), mask_bytes = (size_t)blocks * 4u * 8u, base_bytes = align16((size_t)blocks * 4u);
    if (buf) {
        list[0] = (uint32_t *)buf; list[1] = (uint32_t *)(buf + list_bytes);
        x->masks = (unsigned long long *)(buf + 2u * list_bytes);
        x->block_base = (uint32_t *)(buf + 2u * list_bytes + mask_bytes);
        x->count = (uint32_t *)(buf + 2u * list_bytes + mask_bytes + base_bytes);
    }
    return 2u * list_bytes + mask_bytes + base_bytes + 16u;
}

// The schedule: render the active list up to the next evaluation point, apply the rule, compact the survivors; one 4-byte read
// of the survivor count per batch.
int render_adaptive(rt_scene *scene, const rt_camera *camera, const rt_render_params &p, const rt_adaptive_params &a, int32_t max_spp,
                    double *d_sum, int32_t *d_spp, double *d_sum_sq, hipStream_t stream, rt_adaptive_result *out) {
    *out = rt_adaptive_result{};
    HIP_TRY(hipSetDevice(scene->device));
    const int32_t w = camera->image_width, h = camera->image_height;
    const uint32_t n_pix = (uint32_t)w * (uint32_t)h;
    if (max_spp <= 0) { // nothing to trace: every pixel has 0 samples
        HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)n_pix * 3u * sizeof(double), stream));
        if (d_sum_sq) HIP_TRY(hipMemsetAsync(d_sum_sq, 0, (size_t)n_pix * 3u * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(d_spp, 0, (size_t)n_pix * sizeof(int32_t), stream));
        return RT_OK;
    }
    const uint32_t n_list = (uint32_t)tiles_total(w, h) * 64u;
    // scratch: the step's (adaptive_scratch_layout); behind it the squared sums if the caller wants none
    const size_t step_bytes = adaptive_scratch_layout(n_list, nullptr, nullptr, nullptr);
    const size_t sq_bytes = d_sum_sq ? 0u : (size_t)n_pix * 3u * sizeof(double);
    char *buf = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, step_bytes + sq_bytes));
    struct Free { char *b; hipStream_t s; ~Free() { (void)hipStreamSynchronize(s); (void)hipFree(b); (void)hipGetLastError(); } } release{buf, stream};
    uint32_t *list[2];
    AdaptiveScratch x;
    adaptive_scratch_layout(n_list, buf, list, &x);
    double *sq = d_sum_sq ? d_sum_sq : (double *)(buf + step_bytes);
    launch_tile_order_list(w, h, list[0], stream);
    HIP_TRY(hipGetLastError());
    rt_adaptive_result r{};
    uint32_t n_in = n_list, active = n_pix;
    int32_t n_prev = 0;
    for (int64_t k = 0;; ++k) {
        const int64_t next = (int64_t)a.min_spp + k * (int64_t)a.batch_spp;
        const int32_t n_k = next < max_spp ? (int32_t)next : max_spp;
        rt_render_params rp = p;
        rp.sample_begin = n_prev; rp.sample_end = n_k; rp.accumulate = n_prev > 0 ? 1 : 0;
        const PixelList pl{list[k & 1], (int64_t)n_in, sq};
        if (int rc = launch_render(scene, camera, rp, d_sum, stream, nullptr, &pl)) return rc;
        r.samples += (int64_t)active * (n_k - n_prev);
        r.launches++;
        const bool last = n_k >= max_spp;
        launch_adaptive_step(list[k & 1], n_in, n_pix, d_sum, sq, n_k, last ? 1 : 0, a.rel_threshold, a.abs_threshold, d_spp,
                             list[(k + 1) & 1], x, stream);
        HIP_TRY(hipGetLastError());
        uint32_t survivors = 0;
        HIP_TRY(hipMemcpyAsync(&survivors, x.count, sizeof survivors, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (!last) r.converged += (int32_t)(active - survivors);
        active = survivors;
        if (active == 0) break;
        n_in = (active + 63u) & ~63u;
        n_prev = n_k;
    }
    *out = r;
    return RT_OK;
}

int resolve_scene_options(const rt_scene_options *options, rt_scene_options &opt, const char *who) {
    rt_scene_options_init(&opt);
    if (options) {
        const uint32_t size = options->struct_size;
        if (size < 8 || size > sizeof opt || size % 4 != 0) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": rt_scene_options.struct_size is not one this library knows");
        memcpy(&opt, options, size); // (an older, shorter struct: the fields it lacks keep their defaults)
        opt.struct_size = (uint32_t)sizeof opt;
        // the 56-byte struct of round 2 ended in a reserved word that its init zeroed, where flat_max (0: off) now is
        if (size <= 56) opt.flat_max = -1;
    }
    if (opt.walk < RT_WALK_DEFAULT || opt.walk > RT_WALK_OWN_TREES) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown walk");
    return RT_OK;
}
} // namespace rtapi

extern "C" {

const char *rt_last_error(void) { return g_last_error.c_str(); }
const char *rt_version(void) { return "rt_amd 0.4 (gfx950, abi 2: rt_scene_options grew to 88 bytes, older sizes accepted)"; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int64_t rt_out_size(int32_t width, int32_t height, int32_t out_layout, int32_t shard_index, int32_t shard_count) {
    if (width <= 0 || height <= 0) return -1;
    if (shard_count <= 0) shard_count = 1;
    if (shard_index < 0 || shard_index >= shard_count) return -1;
    if (out_layout == RT_OUT_FRAME) return (int64_t)width * height * 3;
    if (out_layout == RT_OUT_TILES) return tiles_local(width, height, shard_index, shard_count) * RT_TILE_W * RT_TILE_H * 3;
    return -1;
}

void rt_scene_options_init(rt_scene_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->struct_size = (uint32_t)sizeof *o;
    o->walk = RT_WALK_DEFAULT; o->leaf_max = 0; o->refit = -1; o->use_lds = -1;
    o->th_prim = o->th_other = o->th_shade = o->th_box = o->th_new = -1;
    o->sample_buffer_bytes = 0;
    o->reserved_pool = -1;
    o->flat_max = o->start_shortcut = o->defer_instances = o->seq_lookahead = o->slow_min = o->slow_age = o->wide = -1;
    o->quad_filter = -1;
    o->medium_first = -1;
}

// (for a caller compiled against an older, shorter struct: nothing beyond ITS size is written)
int rt_scene_options_init_sized(rt_scene_options *o, uint32_t struct_size) {
    if (!o) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_options_init_sized: null argument");
    if (struct_size < 8 || struct_size > sizeof(rt_scene_options) || struct_size % 4 != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_options_init_sized: struct_size is not one this library knows");
    rt_scene_options full;
    rt_scene_options_init(&full);
    full.struct_size = struct_size;
    memcpy(o, &full, struct_size);
    return RT_OK;
}

int rt_scene_create(const rt_scene_desc *desc, int device, rt_scene **out_scene) { return rt_scene_create_ex(desc, device, nullptr, out_scene); }

int rt_scene_create_ex(const rt_scene_desc *desc, int device, const rt_scene_options *options, rt_scene **out_scene) {
    if (!desc || !out_scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create: null argument");
    *out_scene = nullptr;
    rt_scene_options opt;
    if (int orc = resolve_scene_options(options, opt, "rt_scene_create_ex")) return orc;
    ScenePlan plan; // (a description that does not compile is refused before the device is looked at)
    if (int prc = plan_scene(*desc, opt, tuning_snapshot(), plan, "rt_scene_create")) return prc;
    const int ndev = rt_device_count();
    if (ndev <= 0) return fail(RT_ERR_NO_DEVICE, "rt_scene_create: no HIP device is visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(RT_ERR_NO_DEVICE, "rt_scene_create: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(RT_ERR_HIP, "hipGetDeviceProperties failed");

    std::unique_ptr<rt_scene, void (*)(rt_scene *)> scene(new (std::nothrow) rt_scene(), free_scene);
    if (!scene) return fail(RT_ERR_OUT_OF_MEMORY, "rt_scene_create: out of memory");
    rt_scene *s = scene.get();
    s->device = device;
    s->options = opt;
    s->n_cus = prop.multiProcessorCount;
    s->layout = plan.layout;
    s->stats = plan.stats;
    const Layout &L = s->layout;
    // every table a kernel reads: (wanted, device array <- host vector); the three images only where the plan made them
    struct Upload { bool wanted; int (*run)(rt_scene &, const ScenePlan &); };
    const Upload uploads[] = {
        {L.ordered, [](rt_scene &d, const ScenePlan &p) { return upload(d.oimage, p.oimage); }},
        {L.lds.level != 0, [](rt_scene &d, const ScenePlan &p) { return upload(d.lds_image, p.lds_image); }},
        {L.aux.bytes != 0, [](rt_scene &d, const ScenePlan &p) { return upload(d.aux_image, p.aux_image); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.nodes, p.cs.nodes32); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.oseq, p.cs.oseq); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.spheres, p.cs.spheres); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.quads, p.cs.quads); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.insts, p.cs.instances); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.media, p.cs.media); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.mats, p.mats); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.texs, p.cs.textures); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.perlins, p.cs.perlins); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.images, p.cs.images); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.texels, p.cs.texels); }},
        {true, [](rt_scene &d, const ScenePlan &p) { return upload(d.lut, p.cs.srgb_lut); }},
    };
    for (const Upload &u : uploads)
        if (u.wanted)
            if (int urc = u.run(*s, plan)) return urc;
    // every kernel a render of this scene may launch — dense, its instrumented twin, the list and the views twin — gets its LDS
    // attribute set and its own occupancy figure: the twins are code objects of their own, with their own register counts
    for (int lds = 0; lds < 4; ++lds)
        for (int variant = 0; variant < 4; ++variant) {
            if (lds && lds != L.lds.level) { s->blocks_per_cu[lds][variant] = 0; continue; }
            const bool counted = variant == 1;
            const int jobs = variant == 3 ? JOBS_VIEWS : variant == 2 ? JOBS_LIST : JOBS_DENSE;
            const void *fn = path_kernel_for(lds, counted, kernel_features_for(L.features, lds, L.ordered), L.ordered, aux_in_lds(L, lds), L.wide, jobs);
            const int threads = block_threads(L, lds);
            const size_t dyn = dynamic_lds_bytes(L, lds, counted);
            if (dyn > 48 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
            int b = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, fn, threads, dyn) != hipSuccess || b < 1) b = 1;
            s->blocks_per_cu[lds][variant] = b;
        }
    *out_scene = scene.release();
    return RT_OK;
}

void rt_scene_destroy(rt_scene *scene) { free_scene(scene); }

int rt_scene_get_stats(const rt_scene *scene, rt_scene_stats *out) {
    if (!scene || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_get_stats: null argument");
    *out = scene->stats;
    return RT_OK;
}

int rt_render_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *d_out_rgb_sum,
                     void *hip_stream) {
    if (!scene || !camera || !params || !d_out_rgb_sum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_device: null argument");
    return launch_render(const_cast<rt_scene *>(scene), camera, *params, d_out_rgb_sum, (hipStream_t)hip_stream, nullptr);
}

int rt_render_device_counted(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                             double *d_out_rgb_sum, void *hip_stream, rt_counters *out_counters) {
    if (!scene || !camera || !params || !d_out_rgb_sum || !out_counters)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_device_counted: null argument");
    return launch_render(const_cast<rt_scene *>(scene), camera, *params, d_out_rgb_sum, (hipStream_t)hip_stream, out_counters);
}

int rt_render(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *out_rgb_sum) {
    if (!scene || !camera || !params || !out_rgb_sum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render: null argument");
    rt_render_params p = *params;
    int rc = normalise_params(camera, p);
    if (rc != RT_OK) return rc;
    const int32_t w = camera->image_width, h = camera->image_height;
    const int64_t n_vals = rt_out_size(w, h, RT_OUT_TILES, p.shard_index, p.shard_count);
    if (n_vals <= 0) return RT_OK;
    // on the device the shard always renders into its compact tile buffer; the frame layout is produced on the host, around a staged
    // copy of the tiles (only the pixels of this shard's tiles are read or written in the caller's frame)
    rt_render_params dp = p;
    dp.out_layout = RT_OUT_TILES;
    const bool frame = p.out_layout == RT_OUT_FRAME;
    std::vector<double> tiles(frame ? (size_t)n_vals : 0u);
    if (frame && p.accumulate) // seed the tiles with the caller's running sums
        for_each_shard_pixel(w, h, p.shard_index, p.shard_count, [&](size_t t, size_t f) { std::copy_n(out_rgb_sum + f, 3, &tiles[t]); });
    rt_scene *s = const_cast<rt_scene *>(scene);
    const HostPart parts[] = {{frame ? tiles.data() : out_rgb_sum, (size_t)n_vals * sizeof(double), p.accumulate != 0}};
    rc = render_staged("rt_render", s, true, parts, [&](void *const *d) { return launch_render(s, camera, dp, (double *)d[0], nullptr, nullptr); });
    if (rc == RT_OK && frame)
        for_each_shard_pixel(w, h, p.shard_index, p.shard_count, [&](size_t t, size_t f) { std::copy_n(&tiles[t], 3, out_rgb_sum + f); });
    return rc;
}

// the frame-end kernels run on the device that owns the buffers, whichever device the calling thread had selected
static int select_device_of(const void *device_ptr, const char *who) {
    hipPointerAttribute_t attr;
    // (a plain host pointer: an error on some runtimes, success with type "unregistered" and device -1 on others)
    if (hipPointerGetAttributes(&attr, device_ptr) != hipSuccess || attr.type == hipMemoryTypeUnregistered || attr.device < 0) {
        (void)hipGetLastError();
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": not a device pointer");
    }
    HIP_TRY(hipSetDevice(attr.device));
    return RT_OK;
}

int rt_tiles_to_frame_device(int32_t width, int32_t height, int32_t shard_count, const double *d_gathered, double *d_frame,
                             void *hip_stream) {
    if (!d_gathered || !d_frame || width <= 0 || height <= 0 || shard_count <= 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_tiles_to_frame_device: bad argument");
    if (int rc = select_device_of(d_frame, "rt_tiles_to_frame_device")) return rc;
    const int64_t stride = rt_out_size(width, height, RT_OUT_TILES, 0, shard_count);
    const int32_t tiles_x = (width + RT_TILE_W - 1) / RT_TILE_W;
    launch_tiles_to_frame(width, height, tiles_x, shard_count, stride, d_gathered, d_frame, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
int rt_device_malloc(int device, int64_t bytes, void **out_device_ptr) {
    if (!out_device_ptr || bytes <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_device_malloc: bad argument");
    *out_device_ptr = nullptr;
    if (device < 0 || device >= rt_device_count()) return fail(RT_ERR_NO_DEVICE, "rt_device_malloc: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out_device_ptr, (size_t)bytes));
    return RT_OK;
}

int rt_device_free(int device, void *device_ptr) {
    if (!device_ptr) return RT_OK;
    if (device < 0 || device >= rt_device_count()) return fail(RT_ERR_NO_DEVICE, "rt_device_free: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(device_ptr));
    return RT_OK;
}

int rt_device_download(int device, void *dst_host, const void *src_device, int64_t bytes, void *hip_stream) {
    if (!dst_host || !src_device || bytes <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_device_download: bad argument");
    if (device < 0 || device >= rt_device_count()) return fail(RT_ERR_NO_DEVICE, "rt_device_download: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(dst_host, src_device, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return RT_OK;
}

int rt_device_upload(int device, void *dst_device, const void *src_host, int64_t bytes, void *hip_stream) {
    if (!dst_device || !src_host || bytes <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_device_upload: bad argument");
    if (device < 0 || device >= rt_device_count()) return fail(RT_ERR_NO_DEVICE, "rt_device_upload: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpyAsync(dst_device, src_host, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    return RT_OK;
}

int rt_tiles_to_frame_rgb8_device(int32_t width, int32_t height, int32_t shard_count, const uint8_t *d_gathered, uint8_t *d_frame,
                                  void *hip_stream) {
    if (!d_gathered || !d_frame || width <= 0 || height <= 0 || shard_count <= 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_tiles_to_frame_rgb8_device: bad argument");
    if (int rc = select_device_of(d_frame, "rt_tiles_to_frame_rgb8_device")) return rc;
    const int64_t stride = rt_out_size(width, height, RT_OUT_TILES, 0, shard_count);
    const int32_t tiles_x = (width + RT_TILE_W - 1) / RT_TILE_W;
    launch_tiles_to_frame_rgb8(width, height, tiles_x, shard_count, stride, d_gathered, d_frame, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_resolve_rgb8_values_device(int64_t n_values, int32_t spp, const double *d_sum, uint8_t *d_rgb8, void *hip_stream) {
    if (!d_sum || !d_rgb8 || n_values <= 0 || spp <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_resolve_rgb8_values_device: bad argument");
    if (int rc = select_device_of(d_rgb8, "rt_resolve_rgb8_values_device")) return rc;
    launch_resolve_rgb8(n_values, 1.0 / (double)spp, d_sum, d_rgb8, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_resolve_rgb8_device(int32_t width, int32_t height, int32_t spp, const double *d_frame_sum, uint8_t *d_rgb8, void *hip_stream) {
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_resolve_rgb8_device: bad argument");
    return rt_resolve_rgb8_values_device((int64_t)width * height * 3, spp, d_frame_sum, d_rgb8, hip_stream);
}


// ---- adaptive sampling ------------------------------------------------------------------------------------------------------

int rt_adaptive_params_init_sized(rt_adaptive_params *a, uint32_t struct_size) {
    if (!a) return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_params_init_sized: null argument");
    if (struct_size < 8 || struct_size > sizeof(rt_adaptive_params) || struct_size % 4 != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_params_init_sized: struct_size is not one this library knows");
    rt_adaptive_params full;
    adaptive_defaults(full);
    full.struct_size = struct_size;
    memcpy(a, &full, struct_size);
    return RT_OK;
}

int rt_render_pixels_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const uint32_t *d_pixels,
                            int32_t n_pixels, double *d_sum, double *d_sum_sq, void *hip_stream) {
    if (!scene || !camera || !params || !d_pixels || !d_sum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_pixels_device: null argument");
    if (n_pixels < 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_pixels_device: n_pixels is negative");
    if (n_pixels == 0) return RT_OK;
    const PixelList list{d_pixels, n_pixels, d_sum_sq};
    return launch_render(const_cast<rt_scene *>(scene), camera, *params, d_sum, (hipStream_t)hip_stream, nullptr, &list);
}

// ---- views: many cameras, one launch ----
namespace {
// What the job arithmetic holds, at the one sample per launch that chunking can always fall back to: a job's row (local tile x sample)
// below 2^27 for the exact reciprocal decode, and n_jobs = 64 rows below what launch_render puts into one launch.
constexpr int64_t VIEWS_MAX_ROWS = (int64_t)1 << 27, VIEWS_MAX_JOBS = MAX_JOBS_PER_LAUNCH;
constexpr int64_t VIEWS_MAX_TILES = (VIEWS_MAX_ROWS < VIEWS_MAX_JOBS / 64 ? VIEWS_MAX_ROWS : VIEWS_MAX_JOBS / 64) - 1; // n_views x tiles per frame at most
static_assert(VIEWS_MAX_TILES + 1 == RT_VIEWS_MAX_TILES, "rt_amd.h states the bound");

// every check of the four views entry points, none of which needs a device: the null arguments first (`sq_name`: the squares' buffer, which
// a moments form must be given; `plain`: the entry point that renders without them).  Fills the records.
int check_views(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, const void *out, const char *out_name,
                const char *who, std::vector<ViewRec> &recs, const void *sq = nullptr, const char *sq_name = nullptr, const char *plain = nullptr) {
    const std::string w(who);
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, w + ": scene is null");
    if (!views) return fail(RT_ERR_INVALID_ARGUMENT, w + ": views is null");
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, w + ": params is null");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + out_name + " is null");
    if (sq_name && !sq) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + sq_name + " is null (" + plain + " renders without squares)");
    g_last_launch[0] = 0; // (rt_debug_last_launch: a call that is refused from here on has launched nothing)
    if (n_views < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": n_views must be at least 1");
    if (params->shard_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": shard_count must be 1 (views are not sharded)");
    if (params->out_layout != RT_OUT_FRAME) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_layout must be RT_OUT_FRAME");
    const rt_camera &c0 = views[0].camera;
    if (c0.image_width <= 0 || c0.image_height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": empty image");
    const int64_t tiles = tiles_total(c0.image_width, c0.image_height);
    // (before the loop over the views: a count this large need not have that many entries behind it)
    if ((int64_t)n_views > VIEWS_MAX_TILES / tiles)
        return fail(RT_ERR_UNSUPPORTED, w + ": n_views x tiles per frame exceeds " + std::to_string(VIEWS_MAX_TILES) + " (the job index's 32 bits)");
    for (int32_t v = 1; v < n_views; ++v) {
        const rt_camera &c = views[v].camera;
        const std::string at = w + ": views[" + std::to_string(v) + "].camera.";
        if (c.image_width != c0.image_width) return fail(RT_ERR_INVALID_ARGUMENT, at + "image_width differs from view 0's");
        if (c.image_height != c0.image_height) return fail(RT_ERR_INVALID_ARGUMENT, at + "image_height differs from view 0's");
        if (params->sample_end <= 0 && c.samples_per_pixel != c0.samples_per_pixel)
            return fail(RT_ERR_INVALID_ARGUMENT, at + "samples_per_pixel differs from view 0's and params->sample_end does not set it");
        if (params->max_depth <= 0 && c.max_depth != c0.max_depth)
            return fail(RT_ERR_INVALID_ARGUMENT, at + "max_depth differs from view 0's and params->max_depth does not set it");
    }
    recs.resize((size_t)n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        memset(&recs[(size_t)v], 0, sizeof(ViewRec));
        recs[(size_t)v].cam = views[v].camera;
        recs[(size_t)v].seed_mixed = host_mix64(views[v].seed + 0x9E3779B97F4A7C15ull);
    }
    return RT_OK;
}

// the views' launch: one frame of sums per view at d_out and, with d_sum_sq, one of sums of squares beside it
int launch_views(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, const std::vector<ViewRec> &recs,
                 double *d_out, double *d_sum_sq, hipStream_t stream) {
    rt_render_params p = *params;
    p.shard_index = 0; p.shard_count = 1;
    const ViewTable table{recs.data(), n_views, d_sum_sq};
    return launch_render(const_cast<rt_scene *>(scene), &views[0].camera, p, d_out, stream, nullptr, nullptr, &table);
}
size_t views_bytes(const rt_view *views, int32_t n_views) {
    return (size_t)n_views * (size_t)views[0].camera.image_width * (size_t)views[0].camera.image_height * 3u * sizeof(double);
}
} // namespace

int rt_render_views_device(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, double *d_out,
                           void *hip_stream) {
    std::vector<ViewRec> recs;
    if (int rc = check_views(scene, views, n_views, params, d_out, "d_out", "rt_render_views_device", recs)) return rc;
    return launch_views(scene, views, n_views, params, recs, d_out, nullptr, (hipStream_t)hip_stream);
}

int rt_render_views(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, double *out) {
    std::vector<ViewRec> recs;
    if (int rc = check_views(scene, views, n_views, params, out, "out", "rt_render_views", recs)) return rc;
    const HostPart parts[] = {{out, views_bytes(views, n_views), params->accumulate != 0}};
    return render_staged("rt_render_views", const_cast<rt_scene *>(scene), true, parts, [&](void *const *d) {
        return launch_views(scene, views, n_views, params, recs, (double *)d[0], nullptr, nullptr);
    });
}

// ---- views moments: rt_render_views_device with the sums of squares beside the sums (sum_view_moments_samples_kernel) ----
int rt_render_views_moments_device(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, double *d_sum,
                                   double *d_sum_sq, void *hip_stream) {
    std::vector<ViewRec> recs;
    if (int rc = check_views(scene, views, n_views, params, d_sum, "d_sum", "rt_render_views_moments_device", recs, d_sum_sq, "d_sum_sq", "rt_render_views_device"))
        return rc;
    return launch_views(scene, views, n_views, params, recs, d_sum, d_sum_sq, (hipStream_t)hip_stream);
}

int rt_render_views_moments(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params, double *sum,
                            double *sum_sq) {
    std::vector<ViewRec> recs;
    if (int rc = check_views(scene, views, n_views, params, sum, "sum", "rt_render_views_moments", recs, sum_sq, "sum_sq", "rt_render_views")) return rc;
    const bool running = params->accumulate != 0;
    const HostPart parts[] = {{sum, views_bytes(views, n_views), running}, {sum_sq, views_bytes(views, n_views), running}};
    return render_staged("rt_render_views_moments", const_cast<rt_scene *>(scene), true, parts, [&](void *const *d) {
        return launch_views(scene, views, n_views, params, recs, (double *)d[0], (double *)d[1], nullptr);
    });
}

int rt_render_adaptive_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                              const rt_adaptive_params *adaptive, double *d_sum, int32_t *d_spp, double *d_sum_sq, void *hip_stream,
                              rt_adaptive_result *out_result) {
    const char *who = "rt_render_adaptive_device";
    rt_adaptive_params a;
    rt_render_params p;
    int32_t max_spp = 0;
    if (int rc = check_adaptive(camera, params, adaptive, who, a, p, max_spp)) return rc;
    if (!d_sum) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_sum is null");
    if (!d_spp) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": d_spp is null");
    if (!out_result) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": out_result is null");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": scene is null");
    return render_adaptive(const_cast<rt_scene *>(scene), camera, p, a, max_spp, d_sum, d_spp, d_sum_sq, (hipStream_t)hip_stream, out_result);
}

int rt_render_adaptive(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const rt_adaptive_params *adaptive,
                       double *out_rgb_sum, int32_t *out_spp, double *out_rgb_sum_sq, rt_adaptive_result *out_result) {
    const char *who = "rt_render_adaptive";
    rt_adaptive_params a;
    rt_render_params p;
    int32_t max_spp = 0;
    if (int rc = check_adaptive(camera, params, adaptive, who, a, p, max_spp)) return rc;
    if (!out_rgb_sum) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": out_rgb_sum is null");
    if (!out_spp) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": out_spp is null");
    if (!out_result) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": out_result is null");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": scene is null");
    rt_scene *s = const_cast<rt_scene *>(scene);
    const size_t n_pix = (size_t)camera->image_width * (size_t)camera->image_height, sum_bytes = n_pix * 3u * sizeof(double);
    const HostPart parts[] = {{out_rgb_sum, sum_bytes, false}, {out_rgb_sum_sq, sum_bytes, false}, {out_spp, n_pix * sizeof(int32_t), false}};
    // (not serialised: render_adaptive owns its scratch, and concurrent adaptive calls on one scene have always run side by side)
    return render_staged(who, s, false, parts, [&](void *const *d) {
        return render_adaptive(s, camera, p, a, max_spp, (double *)d[0], (int32_t *)d[2], (double *)d[1], nullptr, out_result);
    });
}

// ---- live refinement: running-mean frames and their display bytes ----
namespace {
// every check of rt_render_mean / rt_render_mean_device and, with `m2_name` (the M2 frame's name: it must not be null then), of
// rt_render_mean_moments / rt_render_mean_moments_device: none needs the scene handle or a device.  Fills the normalised parameters.
static int check_mean(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const void *mean, const char *mean_name,
               const void *rgba8, const char *rgba8_name, const char *who, rt_render_params &p, const void *m2 = nullptr,
               const char *m2_name = nullptr) {
    const std::string w(who);
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, w + ": camera is null");
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, w + ": params is null");
    if (!mean) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + mean_name + " is null");
    if (m2_name && !m2) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + m2_name + " is null");
    p = *params;
    if (p.accumulate != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": accumulate must be 0 (a running mean continues through sample_begin)");
    if (p.shard_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": shard_count must be 1 (the live frame is rendered on one device)");
    if (p.out_layout != RT_OUT_FRAME) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_layout must be RT_OUT_FRAME");
    if (p.sample_begin < 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": sample_begin must not be negative");
    if ((p.sample_end <= 0 ? camera->samples_per_pixel : p.sample_end) <= p.sample_begin)
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": the range [sample_begin, sample_end) is empty");
    p.shard_index = 0; p.shard_count = 1;
    if (int rc = normalise_params(camera, p)) return rc;
    if (((uintptr_t)rgba8 & 3u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + rgba8_name + " must be 4-byte aligned");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, w + ": scene is null");
    return RT_OK;
}
} // namespace

int rt_render_mean_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *d_mean, uint8_t *d_rgba8,
                          void *hip_stream) {
    rt_render_params p;
    if (int rc = check_mean(scene, camera, params, d_mean, "d_mean", d_rgba8, "d_rgba8", "rt_render_mean_device", p)) return rc;
    g_last_launch[0] = 0;
    const MeanOut mean{d_rgba8, nullptr};
    return launch_render(const_cast<rt_scene *>(scene), camera, p, d_mean, (hipStream_t)hip_stream, nullptr, nullptr, nullptr, &mean);
}

int rt_render_mean_moments_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *d_mean, double *d_m2,
                                  uint8_t *d_rgba8, void *hip_stream) {
    rt_render_params p;
    if (int rc = check_mean(scene, camera, params, d_mean, "d_mean", d_rgba8, "d_rgba8", "rt_render_mean_moments_device", p, d_m2, "d_m2")) return rc;
    g_last_launch[0] = 0;
    const MeanOut mean{d_rgba8, d_m2};
    return launch_render(const_cast<rt_scene *>(scene), camera, p, d_mean, (hipStream_t)hip_stream, nullptr, nullptr, nullptr, &mean);
}

namespace {
// rt_render_mean and, with `m2`, rt_render_mean_moments, past their checks: the frames staged as mean | M2 | display bytes, the first two
// uploaded when the call continues them
int render_mean_host(const char *who, rt_scene *s, const rt_camera *camera, const rt_render_params &p, double *mean, double *m2, uint8_t *rgba8) {
    const size_t n_pix = (size_t)camera->image_width * (size_t)camera->image_height, mean_bytes = n_pix * 3u * sizeof(double);
    const bool running = p.sample_begin > 0;
    const HostPart parts[] = {{mean, mean_bytes, running}, {m2, m2 ? mean_bytes : 0u, running}, {rgba8, rgba8 ? n_pix * 4u : 0u, false}};
    return render_staged(who, s, true, parts, [&](void *const *d) {
        const MeanOut out{(uint8_t *)d[2], (double *)d[1]};
        return launch_render(s, camera, p, (double *)d[0], nullptr, nullptr, nullptr, nullptr, &out);
    });
}
} // namespace

int rt_render_mean(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *mean, uint8_t *rgba8) {
    const char *who = "rt_render_mean";
    rt_render_params p;
    if (int rc = check_mean(scene, camera, params, mean, "mean", nullptr, "rgba8", who, p)) return rc; // (host bytes: any alignment)
    g_last_launch[0] = 0;
    return render_mean_host(who, const_cast<rt_scene *>(scene), camera, p, mean, nullptr, rgba8);
}

int rt_render_mean_moments(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *mean, double *m2, uint8_t *rgba8) {
    const char *who = "rt_render_mean_moments";
    rt_render_params p;
    if (int rc = check_mean(scene, camera, params, mean, "mean", nullptr, "rgba8", who, p, m2, "m2")) return rc; // (host bytes: any alignment)
    g_last_launch[0] = 0;
    return render_mean_host(who, const_cast<rt_scene *>(scene), camera, p, mean, m2, rgba8);
}

int rt_resolve_rgba8_device(int32_t width, int32_t height, const double *d_mean, uint8_t *d_rgba8, void *hip_stream) {
    if (!d_mean || !d_rgba8 || width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_resolve_rgba8_device: bad argument");
    if (((uintptr_t)d_rgba8 & 3u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_resolve_rgba8_device: d_rgba8 must be 4-byte aligned");
    if (int rc = select_device_of(d_rgba8, "rt_resolve_rgba8_device")) return rc;
    launch_resolve_rgba8((int64_t)width * height, d_mean, d_rgba8, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- denoise: moments of a whole frame, and the à-trous filter (rt_denoise.hip) ----
namespace {
constexpr size_t MAX_TILE_LISTS = 8; // frame sizes a scene keeps the all-pixels list of

// every check of rt_render_moments / rt_render_moments_device: none needs the scene handle or a device
int check_moments(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const void *sum, const char *sum_name,
                  const void *sum_sq, const char *sum_sq_name, const char *who) {
    const std::string w(who);
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, w + ": camera is null");
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, w + ": params is null");
    if (!sum) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + sum_name + " is null");
    if (!sum_sq) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + sum_sq_name + " is null");
    if (params->shard_count > 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": shard_count must be 1 (the moments are rendered on one device)");
    if (params->out_layout != RT_OUT_FRAME) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_layout must be RT_OUT_FRAME");
    rt_render_params p = *params;
    p.shard_index = 0; p.shard_count = 1;
    if (int rc = normalise_params(camera, p)) return rc;
    if ((int64_t)camera->image_width * camera->image_height >= ((int64_t)1 << 27))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": image_width x image_height must be below 2^27 pixels");
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, w + ": scene is null");
    return RT_OK;
}

// The list of every pixel of a w x h frame in tile order (the first list of rt_render_adaptive), kept by the scene per frame size:
// built once, on `stream`, and waited for there, so that calls on other streams find it complete.  A scene that has seen
// MAX_TILE_LISTS sizes drops them all (after the device has drained) before it keeps another.
int tile_list_of(rt_scene *s, int32_t w, int32_t h, hipStream_t stream, const uint32_t **out, uint32_t *n_list) {
    *n_list = (uint32_t)tiles_total(w, h) * 64u;
    std::lock_guard<std::mutex> lock(s->mu);
    const auto key = std::make_pair(w, h);
    const auto it = s->tile_lists.find(key);
    if (it != s->tile_lists.end()) {
        *out = it->second;
        return RT_OK;
    }
    if (s->tile_lists.size() >= MAX_TILE_LISTS) {
        HIP_TRY(hipDeviceSynchronize());
        for (auto &kv : s->tile_lists) (void)hipFree(kv.second);
        s->tile_lists.clear();
    }
    uint32_t *list = nullptr;
    HIP_TRY(hipMalloc((void **)&list, (size_t)*n_list * sizeof(uint32_t)));
    launch_tile_order_list(w, h, list, stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        (void)hipFree(list);
        return fail(RT_ERR_HIP, std::string("rt_render_moments: ") + hipGetErrorString(e));
    }
    s->tile_lists[key] = list;
    *out = list;
    return RT_OK;
}

int render_moments(rt_scene *s, const rt_camera *camera, const rt_render_params *params, double *d_sum, double *d_sum_sq, hipStream_t stream) {
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t *list = nullptr;
    uint32_t n_list = 0;
    if (int rc = tile_list_of(s, camera->image_width, camera->image_height, stream, &list, &n_list)) return rc;
    rt_render_params p = *params;
    p.shard_index = 0; p.shard_count = 1;
    const PixelList pl{list, (int64_t)n_list, d_sum_sq};
    return launch_render(s, camera, p, d_sum, stream, nullptr, &pl);
}

// the params structs of the denoisers (rt_denoise_params, rt_denoise_albedo_params = its fields and two more, and
// rt_denoise_guided_params = those and sigma_edge): defaults, the
// struct sizes this library knows, the body of *_params_init_sized.  (Templates: C++ linkage inside this file's extern "C".)
extern "C++" {
inline void denoise_defaults(rt_denoise_spatial_params &d) { // (DESIGN.md section 5 "Spatial variance": the CPU sweep)
    memset(&d, 0, sizeof d);
    d.struct_size = (uint32_t)sizeof d;
    d.spatial_below = 2;
    d.window_radius = 1;
}
template <class P> void denoise_defaults(P &d) {
    memset(&d, 0, sizeof d);
    d.struct_size = (uint32_t)sizeof d;
    d.iterations = 4;
    d.sigma = 4.0;
    d.eps = 1e-6;
    if constexpr (std::is_same_v<P, rt_denoise_albedo_params> || std::is_same_v<P, rt_denoise_guided_params>) {
        d.sigma_albedo = 0.5; // (DESIGN.md section 5 "Albedo-guided denoise": the CPU sweep)
        d.albedo_floor = 1e-3;
    }
    if constexpr (std::is_same_v<P, rt_denoise_guided_params>) d.sigma_edge = 0.5; // (DESIGN.md section 5 "Edge-guided denoise")
}
template <class P> bool denoise_size_known(uint32_t size) {
    if constexpr (std::is_same_v<P, rt_denoise_spatial_params>) return size >= 8 && size <= sizeof(P) && size % 4 == 0; // (its fields are words)
    else return size >= 8 && size <= sizeof(P) && size % 8 == 0;
}
// the body of every *_params_init_sized of the frame-end stages, over a stage's own size_known and defaults
template <class P> int params_init_sized(P *params, uint32_t struct_size, const char *who, bool (*size_known)(uint32_t), void (*defaults)(P &)) {
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (!size_known(struct_size)) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": struct_size is not one this library knows");
    P full;
    defaults(full);
    full.struct_size = struct_size;
    memcpy(params, &full, struct_size);
    return RT_OK;
}
template <class P> int denoise_params_init_sized(P *params, uint32_t struct_size, const char *who) {
    return params_init_sized<P>(params, struct_size, who, denoise_size_known<P>, denoise_defaults);
}
// an entry point's params resolved into d: the defaults, and over them the caller's struct as far as it goes (an older, shorter struct:
// the fields it lacks keep their defaults).  False: its struct_size is not one this library knows
template <class P> bool denoise_params_resolve(const P *params, P &d) {
    denoise_defaults(d);
    if (!params) return true;
    if (!denoise_size_known<P>(params->struct_size)) return false;
    memcpy(&d, params, params->struct_size);
    return true;
}
} // extern "C++"
int64_t denoise_workspace_bytes(int32_t width, int32_t height, int regions) { // regions of 4 doubles per pixel
    if (width <= 0 || height <= 0 || (int64_t)width * height >= ((int64_t)1 << 27)) return -1;
    return (int64_t)width * height * regions * 4 * (int64_t)sizeof(double);
}
// the views forms': n_views times the single-frame figure; -1 for what the call refuses or (no n_views the call takes gets there) what
// does not fit an int64
int64_t denoise_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views, int regions) {
    const int64_t one = denoise_workspace_bytes(width, height, regions);
    if (one < 0 || n_views < 1 || n_views > RT_DENOISE_MAX_VIEWS) return -1;
    int64_t all = 0;
    if (__builtin_mul_overflow(one, (int64_t)n_views, &all)) return -1;
    return all;
}
bool overlaps(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every denoise entry point is one DenoiseCall handed to run_denoise: every check in the header's order, each message under the caller's
// name `who` and with the inputs named as the caller names them, then prepare and the K iterations.  What a call does not have is a null
// pointer or an empty optional.  Each check of the edge guide sits behind the albedo guide's of the same kind.
enum class DenoiseInput { Sums, Means }; // sums and sums of squares with a count or a map, or running means and M2 after `count` samples
struct GuideFrame {
    const double *frame; // 3 w h doubles per view, null is refused: sums of `count` samples or, in the means forms, means
    double count;        // the divisor (means forms: 1.0, neither read nor checked)
};
struct SpatialRoute { // with count < spatial_below the spatial prepare runs in the elementwise one's place, and `second` may be null
    rt_denoise_spatial_params params;
    bool known; // its struct_size is one this library knows
};
struct DenoiseCall {
    const char *who;
    DenoiseInput form;
    int32_t width, height;
    std::optional<int32_t> n_views; // the views forms: a stack, view-major in every buffer and every region of the workspace, filtered in the same K + 1 launches
    const double *first, *second;   // d_sum and d_sum_sq, or d_mean and d_m2
    int32_t count;                  // spp, or samples
    const int32_t *spp_map;         // sums form, or null
    std::optional<GuideFrame> albedo, edge;
    std::optional<SpatialRoute> spatial; // the *_mean_spatial entry points
    rt_denoise_guided_params filter;     // the caller's params over the defaults, as denoise_with resolved them; refused in their place among the checks
    bool filter_known;                   // if their struct_size was not known
    const char *filter_name;             // the C name of the struct that arrived
    double *out;
    uint8_t *rgba8;
    void *workspace, *stream;
};
int run_denoise(const DenoiseCall &c) {
    const std::string w(c.who);
    const bool means = c.form == DenoiseInput::Means;
    const char *first = means ? "d_mean" : "d_sum", *second = means ? "d_m2" : "d_sum_sq", *third = means ? "d_albedo_mean" : "d_albedo_sum",
               *fourth = means ? "d_edge_mean" : "d_edge_sum";
    const rt_denoise_guided_params &d = c.filter;
    const int32_t width = c.width, height = c.height;
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width and height must be positive");
    if ((int64_t)width * height >= ((int64_t)1 << 27)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width x height must be below 2^27 pixels");
    if (c.n_views && *c.n_views < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": n_views must be at least 1");
    if (c.n_views && *c.n_views > RT_DENOISE_MAX_VIEWS)
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": n_views must be at most " + std::to_string(RT_DENOISE_MAX_VIEWS) + " (the launch grid's second dimension)");
    const int32_t n_views = c.n_views.value_or(1);
    if (!c.first) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + first + " is null");
    if (!c.second && !c.spatial) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + second + " is null");
    if (c.albedo && !c.albedo->frame) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + third + " is null");
    if (c.edge && !c.edge->frame) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + fourth + " is null");
    if (!c.out) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_mean_out is null");
    if (!c.workspace) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace is null");
    if (means && c.count < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": samples must be at least 1 (the number of samples in d_mean)");
    if (!means && !c.spp_map && c.count < 2) return fail(RT_ERR_INVALID_ARGUMENT, w + ": spp must be at least 2 (a variance needs two samples)" + (c.n_views ? "" : " when d_spp is null"));
    if (!means && c.albedo && c.albedo->count < 1.0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": albedo_spp must be at least 1");
    if (!means && c.edge && c.edge->count < 1.0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": edge_spp must be at least 1");
    bool spatial_route = false;
    if (c.spatial) {
        const rt_denoise_spatial_params &sp = c.spatial->params;
        if (!c.spatial->known) return fail(RT_ERR_INVALID_ARGUMENT, w + ": rt_denoise_spatial_params.struct_size is not one this library knows");
        if (sp.spatial_below < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": spatial_below must be at least 1");
        if (sp.window_radius < 1 || sp.window_radius > 3) return fail(RT_ERR_INVALID_ARGUMENT, w + ": window_radius must be 1..3");
        spatial_route = c.count < sp.spatial_below;
        if (!spatial_route && !c.second)
            return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + second + " is null (it is read when samples >= spatial_below)");
    }
    if (!c.filter_known) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + c.filter_name + ".struct_size is not one this library knows");
    if (d.iterations < 1 || d.iterations > 6) return fail(RT_ERR_INVALID_ARGUMENT, w + ": iterations must be 1..6");
    if (!(d.sigma > 0.0) || !std::isfinite(d.sigma)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": sigma must be a number > 0");
    if (!(d.eps > 0.0) || !std::isfinite(d.eps)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": eps must be a number > 0");
    if (c.albedo && (!(d.sigma_albedo > 0.0) || !std::isfinite(d.sigma_albedo))) return fail(RT_ERR_INVALID_ARGUMENT, w + ": sigma_albedo must be a number > 0");
    if (c.albedo && (!(d.albedo_floor > 0.0) || !std::isfinite(d.albedo_floor))) return fail(RT_ERR_INVALID_ARGUMENT, w + ": albedo_floor must be a number > 0");
    if (c.edge && (!(d.sigma_edge > 0.0) || !std::isfinite(d.sigma_edge))) return fail(RT_ERR_INVALID_ARGUMENT, w + ": sigma_edge must be a number > 0");
    const size_t n_pix = (size_t)width * (size_t)height, frame_bytes = (size_t)n_views * n_pix * 3u * sizeof(double); // (the whole stack's)
    if (overlaps(c.out, frame_bytes, c.first, frame_bytes) || (c.second && overlaps(c.out, frame_bytes, c.second, frame_bytes)) ||
        (c.albedo && overlaps(c.out, frame_bytes, c.albedo->frame, frame_bytes)))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_mean_out must not overlap " + first + (c.albedo ? std::string(", ") + second + " or " + third : std::string(" or ") + second));
    if (c.edge && overlaps(c.out, frame_bytes, c.edge->frame, frame_bytes)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_mean_out must not overlap " + fourth);
    if (((uintptr_t)c.rgba8 & 3u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_rgba8 must be 4-byte aligned");
    if (((uintptr_t)c.workspace & 15u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    if (int rc = select_device_of(c.out, c.who)) return rc;
    hipStream_t stream = (hipStream_t)c.stream;
    // the workspace: two halves and behind them the guides' regions, the albedo guide's third; the edge guide's is the third alone and the fourth beside it
    const size_t region = (size_t)n_views * n_pix * 4u * sizeof(double);
    char *half[2] = {(char *)c.workspace, (char *)c.workspace + region};
    DenoiseGuide albedo_guide{};
    DenoiseEdge edge_guide{};
    if (c.albedo) albedo_guide = {c.albedo->frame, c.albedo->count, d.albedo_floor, d.sigma_albedo, (double4 *)((char *)c.workspace + 2u * region)};
    if (c.edge) edge_guide = {c.edge->frame, c.edge->count, d.sigma_edge, (double4 *)((char *)c.workspace + (c.albedo ? 3u : 2u) * region)};
    const DenoiseGuide *guide = c.albedo ? &albedo_guide : nullptr;
    const DenoiseEdge *edge = c.edge ? &edge_guide : nullptr;
    if (spatial_route) launch_denoise_prepare_spatial(width, height, c.spatial->params.window_radius, c.first, guide, half[0], stream, edge);
    else launch_denoise_prepare((int64_t)n_pix, n_views, c.first, c.second, c.count, c.spp_map, guide, means, half[0], stream, edge);
    HIP_TRY(hipGetLastError());
    for (int32_t k = 0; k < d.iterations; ++k) {
        const bool last = k == d.iterations - 1;
        launch_denoise_atrous(width, height, n_views, (int32_t)1 << k, d.sigma, d.eps, guide, half[k & 1], last ? nullptr : half[(k + 1) & 1],
                              last ? c.out : nullptr, last ? c.rgba8 : nullptr, stream, edge);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}
// An entry point's call: the caller's filter params — any of the three structs, each the next one's first fields — over the defaults in the
// description, with whether their size was known and the struct's C name; then the description is run.
// (Templates, and what the dynamic symbol table is not to list: C++ linkage inside this file's extern "C".)
extern "C++" {
constexpr const char *denoise_params_name(const rt_denoise_params *) { return "rt_denoise_params"; }
constexpr const char *denoise_params_name(const rt_denoise_albedo_params *) { return "rt_denoise_albedo_params"; }
constexpr const char *denoise_params_name(const rt_denoise_guided_params *) { return "rt_denoise_guided_params"; }
template <class P> int denoise_with(const P *params, DenoiseCall call) {
    static_assert(offsetof(rt_denoise_albedo_params, sigma_albedo) == sizeof(rt_denoise_params) &&
                  offsetof(rt_denoise_guided_params, sigma_edge) == sizeof(rt_denoise_albedo_params), "each params struct extends the one before");
    P d;
    call.filter_known = denoise_params_resolve(params, d);
    call.filter_name = denoise_params_name(params);
    denoise_defaults(call.filter);
    memcpy(&call.filter, &d, sizeof d); // the fields P has
    return run_denoise(call);
}
// rt_denoise_guided_*: the albedo guide is there only with its frame (rt_denoise_albedo_*: always, and a null frame is refused)
std::optional<GuideFrame> guide_if(const double *frame, double count) { return frame ? std::optional<GuideFrame>(GuideFrame{frame, count}) : std::nullopt; }
SpatialRoute spatial_route_of(const rt_denoise_spatial_params *spatial) {
    SpatialRoute route;
    route.known = denoise_params_resolve(spatial, route.params);
    return route;
}
} // extern "C++"
} // namespace

int rt_render_moments_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *d_sum, double *d_sum_sq,
                             void *hip_stream) {
    if (int rc = check_moments(scene, camera, params, d_sum, "d_sum", d_sum_sq, "d_sum_sq", "rt_render_moments_device")) return rc;
    g_last_launch[0] = 0;
    return render_moments(const_cast<rt_scene *>(scene), camera, params, d_sum, d_sum_sq, (hipStream_t)hip_stream);
}

int rt_render_moments(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, double *sum, double *sum_sq) {
    const char *who = "rt_render_moments";
    if (int rc = check_moments(scene, camera, params, sum, "sum", sum_sq, "sum_sq", who)) return rc;
    g_last_launch[0] = 0;
    rt_scene *s = const_cast<rt_scene *>(scene);
    const size_t bytes = (size_t)camera->image_width * (size_t)camera->image_height * 3u * sizeof(double);
    const bool running = params->accumulate != 0;
    const HostPart parts[] = {{sum, bytes, running}, {sum_sq, bytes, running}};
    return render_staged(who, s, true, parts, [&](void *const *d) { return render_moments(s, camera, params, (double *)d[0], (double *)d[1], nullptr); });
}

int rt_denoise_params_init_sized(rt_denoise_params *params, uint32_t struct_size) {
    return denoise_params_init_sized(params, struct_size, "rt_denoise_params_init_sized");
}

int64_t rt_denoise_workspace_bytes(int32_t width, int32_t height) { return denoise_workspace_bytes(width, height, 2); }

int rt_denoise_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                      const rt_denoise_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_device", .form = DenoiseInput::Sums, .width = width, .height = height, .first = d_sum, .second = d_sum_sq,
                                 .count = spp, .spp_map = d_spp, .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int64_t rt_denoise_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views) {
    return denoise_views_workspace_bytes(width, height, n_views, 2);
}

int rt_denoise_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                            const rt_denoise_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_views_device", .form = DenoiseInput::Sums, .width = width, .height = height, .n_views = n_views, .first = d_sum,
                                 .second = d_sum_sq, .count = spp, .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int rt_denoise_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples, const rt_denoise_params *params,
                           double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_mean_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean, .second = d_m2,
                                 .count = samples, .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int rt_denoise_spatial_params_init_sized(rt_denoise_spatial_params *params, uint32_t struct_size) {
    return denoise_params_init_sized(params, struct_size, "rt_denoise_spatial_params_init_sized");
}

int rt_denoise_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                   const rt_denoise_spatial_params *spatial, const rt_denoise_params *params, double *d_mean_out, uint8_t *d_rgba8,
                                   void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_mean_spatial_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean,
                                 .second = d_m2, .count = samples, .spatial = spatial_route_of(spatial), .out = d_mean_out, .rgba8 = d_rgba8,
                                 .workspace = d_workspace, .stream = hip_stream});
}

// ---- albedo scene and the albedo-guided filter (rt_denoise.hip, with a guide) ----
int rt_albedo_materials(const rt_scene_desc *desc, rt_material *out_materials, rt_texture *out_textures, int32_t *out_n_textures) {
    const std::string w("rt_albedo_materials");
    if (!desc) return fail(RT_ERR_INVALID_ARGUMENT, w + ": desc is null");
    if (!out_materials) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_materials is null");
    if (!out_textures) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_textures is null");
    if (!out_n_textures) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_n_textures is null");
    if (desc->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARGUMENT, w + ": abi_version mismatch");
    if (desc->n_materials < 0 || (desc->n_materials > 0 && !desc->materials))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": materials is a null array with a non-zero count, or n_materials is negative");
    if (desc->n_textures < 0 || (desc->n_textures > 0 && !desc->textures))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": textures is a null array with a non-zero count, or n_textures is negative");
    // every check before the first write
    for (int32_t k = 0; k < desc->n_materials; ++k) {
        const rt_material &m = desc->materials[k];
        const std::string at = w + ": materials[" + std::to_string(k) + "]";
        switch (m.kind) {
        case RT_MATERIAL_LAMBERTIAN:
        case RT_MATERIAL_DIFFUSE_LIGHT:
        case RT_MATERIAL_ISOTROPIC:
            if (m.texture < 0 || m.texture >= desc->n_textures) return fail(RT_ERR_INVALID_ARGUMENT, at + ".texture: texture index out of range");
            break;
        case RT_MATERIAL_METAL:
        case RT_MATERIAL_DIELECTRIC: break;
        default: return fail(RT_ERR_INVALID_ARGUMENT, at + ".kind: unknown material kind");
        }
    }
    for (int32_t t = 0; t < desc->n_textures; ++t) out_textures[t] = desc->textures[t];
    int32_t n_tex = desc->n_textures;
    auto solid = [&](const rt_vec3 &colour) {
        rt_texture t;
        memset(&t, 0, sizeof t);
        t.kind = RT_TEXTURE_SOLID;
        t.even = t.odd = t.image = t.perlin = -1;
        t.color = colour;
        out_textures[n_tex] = t;
        return n_tex++;
    };
    for (int32_t k = 0; k < desc->n_materials; ++k) {
        const rt_material &m = desc->materials[k];
        if (m.kind == RT_MATERIAL_DIFFUSE_LIGHT) {
            out_materials[k] = m;
            continue;
        }
        rt_material o;
        memset(&o, 0, sizeof o);
        o.kind = RT_MATERIAL_DIFFUSE_LIGHT;
        if (m.kind == RT_MATERIAL_METAL) o.texture = solid(m.albedo);
        else if (m.kind == RT_MATERIAL_DIELECTRIC) o.texture = solid(rt_vec3{1.0, 1.0, 1.0});
        else o.texture = m.texture;
        out_materials[k] = o;
    }
    *out_n_textures = n_tex;
    return RT_OK;
}

int rt_scene_create_albedo(const rt_scene_desc *desc, int device, const rt_scene_options *options, rt_scene **out_scene) {
    if (!desc || !out_scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create_albedo: null argument");
    *out_scene = nullptr;
    if (desc->n_materials < 0 || desc->n_textures < 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create_albedo: n_materials or n_textures is negative");
    std::vector<rt_material> materials((size_t)desc->n_materials + 1u);
    std::vector<rt_texture> textures((size_t)desc->n_textures + (size_t)desc->n_materials + 1u);
    int32_t n_textures = 0;
    if (int rc = rt_albedo_materials(desc, materials.data(), textures.data(), &n_textures)) return rc;
    rt_scene_desc albedo = *desc;
    albedo.materials = materials.data();
    albedo.textures = textures.data();
    albedo.n_textures = n_textures;
    return rt_scene_create_ex(&albedo, device, options, out_scene);
}

int rt_denoise_albedo_params_init_sized(rt_denoise_albedo_params *params, uint32_t struct_size) {
    return denoise_params_init_sized(params, struct_size, "rt_denoise_albedo_params_init_sized");
}

int64_t rt_denoise_albedo_workspace_bytes(int32_t width, int32_t height) { return denoise_workspace_bytes(width, height, 3); }

int rt_denoise_albedo_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                             const double *d_albedo_sum, int32_t albedo_spp, const rt_denoise_albedo_params *params, double *d_mean_out,
                             uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_albedo_device", .form = DenoiseInput::Sums, .width = width, .height = height, .first = d_sum, .second = d_sum_sq,
                                 .count = spp, .spp_map = d_spp, .albedo = GuideFrame{d_albedo_sum, (double)albedo_spp}, .out = d_mean_out, .rgba8 = d_rgba8,
                                 .workspace = d_workspace, .stream = hip_stream});
}

int64_t rt_denoise_albedo_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views) {
    return denoise_views_workspace_bytes(width, height, n_views, 3);
}

int rt_denoise_albedo_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const double *d_albedo_sum, int32_t albedo_spp, const rt_denoise_albedo_params *params, double *d_mean_out,
                                   uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_albedo_views_device", .form = DenoiseInput::Sums, .width = width, .height = height, .n_views = n_views,
                                 .first = d_sum, .second = d_sum_sq, .count = spp, .albedo = GuideFrame{d_albedo_sum, (double)albedo_spp}, .out = d_mean_out,
                                 .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int rt_denoise_albedo_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples, const double *d_albedo_mean,
                                  const rt_denoise_albedo_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_albedo_mean_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean,
                                 .second = d_m2, .count = samples, .albedo = GuideFrame{d_albedo_mean, 1.0}, .out = d_mean_out, .rgba8 = d_rgba8,
                                 .workspace = d_workspace, .stream = hip_stream});
}

int rt_denoise_albedo_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                          const double *d_albedo_mean, const rt_denoise_spatial_params *spatial, const rt_denoise_albedo_params *params,
                                          double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_albedo_mean_spatial_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean,
                                 .second = d_m2, .count = samples, .albedo = GuideFrame{d_albedo_mean, 1.0}, .spatial = spatial_route_of(spatial), .out = d_mean_out,
                                 .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

// ---- surface-ID scene and the edge-guided filter (rt_denoise.hip, with an edge guide) ----
int rt_surface_id_tables(const rt_scene_desc *desc, rt_sphere *out_spheres, rt_quad *out_quads, rt_constant_medium *out_media, rt_material *out_materials,
                         rt_texture *out_textures) {
    const std::string w("rt_surface_id_tables");
    if (!desc) return fail(RT_ERR_INVALID_ARGUMENT, w + ": desc is null");
    if (!out_spheres) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_spheres is null");
    if (!out_quads) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_quads is null");
    if (!out_media) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_media is null");
    if (!out_materials) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_materials is null");
    if (!out_textures) return fail(RT_ERR_INVALID_ARGUMENT, w + ": out_textures is null");
    if (desc->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID_ARGUMENT, w + ": abi_version mismatch");
    if (desc->n_spheres < 0 || (desc->n_spheres > 0 && !desc->spheres))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": spheres is a null array with a non-zero count, or n_spheres is negative");
    if (desc->n_quads < 0 || (desc->n_quads > 0 && !desc->quads))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": quads is a null array with a non-zero count, or n_quads is negative");
    if (desc->n_media < 0 || (desc->n_media > 0 && !desc->media))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": media is a null array with a non-zero count, or n_media is negative");
    // every check before the first write
    for (int32_t i = 0; i < RT_SURFACE_ID_COLOURS; ++i) {
        const int32_t q = i + 1; // the palette entry: black, q = 0, is not in it
        rt_texture t;
        memset(&t, 0, sizeof t);
        t.kind = RT_TEXTURE_SOLID;
        t.even = t.odd = t.image = t.perlin = -1;
        t.color = rt_vec3{0.5 * (double)(q % 3), 0.5 * (double)((q / 3) % 3), 0.5 * (double)(q / 9)};
        out_textures[i] = t;
        rt_material m;
        memset(&m, 0, sizeof m);
        m.kind = RT_MATERIAL_DIFFUSE_LIGHT;
        m.texture = i;
        out_materials[i] = m;
    }
    int64_t k = 0; // the surface's number: spheres, then quads, then media
    for (int32_t i = 0; i < desc->n_spheres; ++i, ++k) {
        out_spheres[i] = desc->spheres[i];
        out_spheres[i].material = (int32_t)(k % RT_SURFACE_ID_COLOURS);
    }
    for (int32_t i = 0; i < desc->n_quads; ++i, ++k) {
        out_quads[i] = desc->quads[i];
        out_quads[i].material = (int32_t)(k % RT_SURFACE_ID_COLOURS);
    }
    for (int32_t i = 0; i < desc->n_media; ++i, ++k) {
        out_media[i] = desc->media[i];
        out_media[i].phase_material = (int32_t)(k % RT_SURFACE_ID_COLOURS);
    }
    return RT_OK;
}

int rt_scene_create_surface_ids(const rt_scene_desc *desc, int device, const rt_scene_options *options, rt_scene **out_scene) {
    if (!desc || !out_scene) return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create_surface_ids: null argument");
    *out_scene = nullptr;
    if (desc->n_spheres < 0 || desc->n_quads < 0 || desc->n_media < 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_scene_create_surface_ids: n_spheres, n_quads or n_media is negative");
    std::vector<rt_sphere> spheres((size_t)desc->n_spheres + 1u);
    std::vector<rt_quad> quads((size_t)desc->n_quads + 1u);
    std::vector<rt_constant_medium> media((size_t)desc->n_media + 1u);
    std::vector<rt_material> materials(RT_SURFACE_ID_COLOURS);
    std::vector<rt_texture> textures(RT_SURFACE_ID_COLOURS);
    if (int rc = rt_surface_id_tables(desc, spheres.data(), quads.data(), media.data(), materials.data(), textures.data())) return rc;
    rt_scene_desc ids = *desc;
    ids.spheres = spheres.data();
    ids.quads = quads.data();
    ids.media = media.data();
    ids.materials = materials.data();
    ids.textures = textures.data();
    ids.n_materials = ids.n_textures = RT_SURFACE_ID_COLOURS;
    return rt_scene_create_ex(&ids, device, options, out_scene);
}

int rt_denoise_guided_params_init_sized(rt_denoise_guided_params *params, uint32_t struct_size) {
    return denoise_params_init_sized(params, struct_size, "rt_denoise_guided_params_init_sized");
}

int64_t rt_denoise_guided_workspace_bytes(int32_t width, int32_t height, int32_t with_albedo) {
    return denoise_workspace_bytes(width, height, with_albedo ? 4 : 3);
}

int rt_denoise_guided_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                             const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp,
                             const rt_denoise_guided_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_guided_device", .form = DenoiseInput::Sums, .width = width, .height = height, .first = d_sum, .second = d_sum_sq,
                                 .count = spp, .spp_map = d_spp, .albedo = guide_if(d_albedo_sum, albedo_spp), .edge = GuideFrame{d_edge_sum, (double)edge_spp},
                                 .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

// the edge guide on the other routes (include/rt_amd.h "edge guide on every route"): the means, spatial-variance and views forms
int rt_denoise_guided_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples, const double *d_albedo_mean,
                                  const double *d_edge_mean, const rt_denoise_guided_params *params, double *d_mean_out, uint8_t *d_rgba8,
                                  void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_guided_mean_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean,
                                 .second = d_m2, .count = samples, .albedo = guide_if(d_albedo_mean, 1.0), .edge = GuideFrame{d_edge_mean, 1.0}, .out = d_mean_out,
                                 .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int rt_denoise_guided_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                          const double *d_albedo_mean, const double *d_edge_mean, const rt_denoise_spatial_params *spatial,
                                          const rt_denoise_guided_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace,
                                          void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_guided_mean_spatial_device", .form = DenoiseInput::Means, .width = width, .height = height, .first = d_mean,
                                 .second = d_m2, .count = samples, .albedo = guide_if(d_albedo_mean, 1.0), .edge = GuideFrame{d_edge_mean, 1.0},
                                 .spatial = spatial_route_of(spatial), .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

int64_t rt_denoise_guided_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views, int32_t with_albedo) {
    return denoise_views_workspace_bytes(width, height, n_views, with_albedo ? 4 : 3);
}

int rt_denoise_guided_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp,
                                   const rt_denoise_guided_params *params, double *d_mean_out, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return denoise_with(params, {.who = "rt_denoise_guided_views_device", .form = DenoiseInput::Sums, .width = width, .height = height, .n_views = n_views,
                                 .first = d_sum, .second = d_sum_sq, .count = spp, .albedo = guide_if(d_albedo_sum, albedo_spp),
                                 .edge = GuideFrame{d_edge_sum, (double)edge_spp}, .out = d_mean_out, .rgba8 = d_rgba8, .workspace = d_workspace,
                                 .stream = hip_stream});
}

// ---- tone mapping (rt_tonemap.hip): exposure and a tone curve in front of the output stage's gamma, auto-exposure from a device reduction ----

int rt_tonemap_params_init_sized(rt_tonemap_params *params, uint32_t struct_size) {
    return params_init_sized(params, struct_size, "rt_tonemap_params_init_sized", rttm::size_known, rttm::defaults);
}

int64_t rt_tonemap_workspace_bytes(int32_t width, int32_t height) { return rttm::workspace_bytes(width, height); }

// What rt_tonemap_device and rt_film_device are: one frame of values through the exposure and the operator into bytes — the tone-mapping
// stage's RGB8 / RGBA8, or (film != null) one film format.  The checks in the headers' order, the reduction if auto_key > 0, the launches.
struct OutputStageCall {
    const char *who;
    int32_t width, height;
    const double *values;
    int32_t spp;
    const int32_t *spp_map;
    const rt_tonemap_params *params;
    uint8_t *rgb8 = nullptr, *rgba8 = nullptr; // the tone-mapping stage's outputs
    bool film = false;                         // rt_film_device: `out` in `format`
    int32_t format = 0;
    void *out = nullptr;
    void *workspace;
    void *stream;
};

static int output_stage(const OutputStageCall &c) {
    const std::string w(c.who);
    const int32_t width = c.width, height = c.height;
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width and height must be positive");
    if ((int64_t)width * height >= rttm::MAX_PIXELS) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width x height must be below 2^27 pixels");
    if (!c.values) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_values is null");
    if (c.film && !c.out) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_out is null");
    if (!c.film && !c.rgb8 && !c.rgba8) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_rgb8 and d_rgba8 are both null");
    if (c.spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": spp must be at least 1");
    if (c.film && !rttm::film_pixel_bytes(c.format))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": format must be RT_FILM_RGBE, RT_FILM_F32 or RT_FILM_RGB16 (0..2)");
    rt_tonemap_params p;
    if (!rttm::resolve(c.params, p)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": rt_tonemap_params.struct_size is not one this library knows");
    if (const char *bad = rttm::bad_field(p)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    const bool automatic = p.auto_key > 0.0;
    if (automatic && !c.workspace) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace is null (auto_key > 0 needs it)");
    if (automatic && ((uintptr_t)c.workspace & 15u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    if (((uintptr_t)c.rgba8 & 3u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_rgba8 must be 4-byte aligned");
    if (c.film && ((uintptr_t)c.out & (rttm::film_alignment(c.format) - 1u)) != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, w + (c.format == RT_FILM_RGB16 ? ": d_out must be 2-byte aligned" : ": d_out must be 4-byte aligned"));
    const size_t n_pix = (size_t)width * (size_t)height, value_bytes = n_pix * 3u * sizeof(double);
    if (c.film && overlaps(c.out, n_pix * (size_t)rttm::film_pixel_bytes(c.format), c.values, value_bytes))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_out must not overlap d_values");
    if ((c.rgb8 && overlaps(c.rgb8, n_pix * 3u, c.values, value_bytes)) || (c.rgba8 && overlaps(c.rgba8, n_pix * 4u, c.values, value_bytes)))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": an output must not overlap d_values");
    if (int rc = select_device_of(c.film ? c.out : c.rgb8 ? (void *)c.rgb8 : (void *)c.rgba8, c.who)) return rc;
    hipStream_t stream = (hipStream_t)c.stream;
    const double inv_spp = 1.0 / (double)c.spp, w2 = p.white * p.white;
    double *out4 = (double *)c.workspace;
    if (automatic) {
        launch_log_average((int64_t)n_pix, c.values, inv_spp, c.spp_map, p.delta, (TonemapPartial *)(out4 + 4), p.exposure, p.auto_key, out4, stream);
        HIP_TRY(hipGetLastError());
    }
    const double *d_scale = automatic ? out4 + 3 : nullptr;
    if (c.film) {
        launch_film(c.format, (int64_t)n_pix, c.values, inv_spp, c.spp_map, p.exposure, d_scale, p.op, w2, c.out, stream);
        HIP_TRY(hipGetLastError());
    }
    if (c.rgb8) {
        launch_tonemap_rgb8((int64_t)n_pix, c.values, inv_spp, c.spp_map, p.exposure, d_scale, p.op, w2, c.rgb8, stream);
        HIP_TRY(hipGetLastError());
    }
    if (c.rgba8) {
        launch_tonemap_rgba8((int64_t)n_pix, c.values, inv_spp, c.spp_map, p.exposure, d_scale, p.op, w2, c.rgba8, stream);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int rt_tonemap_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const rt_tonemap_params *params,
                      uint8_t *d_rgb8, uint8_t *d_rgba8, void *d_workspace, void *hip_stream) {
    return output_stage({.who = "rt_tonemap_device", .width = width, .height = height, .values = d_values, .spp = spp, .spp_map = d_spp, .params = params,
                         .rgb8 = d_rgb8, .rgba8 = d_rgba8, .workspace = d_workspace, .stream = hip_stream});
}

// ---- film output (rt_film.hip): the tone-mapping stage's value in a file's format — shared-exponent RGBE, f32 or 16-bit gamma ----

int64_t rt_film_bytes(int32_t width, int32_t height, int32_t format) { return rttm::film_bytes(width, height, format); }

int rt_film_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const rt_tonemap_params *tone,
                   int32_t format, void *d_out, void *d_workspace, void *hip_stream) {
    return output_stage({.who = "rt_film_device", .width = width, .height = height, .values = d_values, .spp = spp, .spp_map = d_spp, .params = tone,
                         .film = true, .format = format, .out = d_out, .workspace = d_workspace, .stream = hip_stream});
}

int rt_log_average_luminance_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, double delta,
                                    double *d_out4, void *d_workspace, void *hip_stream) {
    const std::string w("rt_log_average_luminance_device");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width and height must be positive");
    if ((int64_t)width * height >= rttm::MAX_PIXELS) return fail(RT_ERR_INVALID_ARGUMENT, w + ": width x height must be below 2^27 pixels");
    if (!d_values) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_values is null");
    if (!d_out4) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_out4 is null");
    if (spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, w + ": spp must be at least 1");
    if (!rttm::positive_finite(delta)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": delta must be a finite number > 0");
    if (!d_workspace) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace is null");
    if (((uintptr_t)d_workspace & 15u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    const size_t n_pix = (size_t)width * (size_t)height;
    if (overlaps(d_out4, 4u * sizeof(double), d_values, n_pix * 3u * sizeof(double))) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_out4 must not overlap d_values");
    if (int rc = select_device_of(d_out4, "rt_log_average_luminance_device")) return rc;
    // (the workspace's own four result doubles are not used by this call: the levels' blocks start behind them, as in rt_tonemap_device)
    launch_log_average((int64_t)n_pix, d_values, 1.0 / (double)spp, d_spp, delta, (TonemapPartial *)((double *)d_workspace + 4), 1.0, 0.0, d_out4,
                       (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- bloom (rt_bloom.hip): a bright pass and K a-trous levels of the B3-spline blur, their average added back to the means ----

// The largest stride whose level runs as the one-launch LDS form; negative: the built-in rule (rt_debug_set_bloom_fused; speed only).
// The rule is DESIGN.md "Bloom"'s measurement: strides 1 and 2 where the frame has at least two tiles per CU of an MI355X — the form is
// 5 % ahead on 1200 x 800 (950 tiles) and well behind on 256 x 256 (64 tiles), where its workgroups cannot fill the machine.
constexpr int64_t BLOOM_FUSED_MIN_TILES = 512;
static std::atomic<int32_t> g_bloom_fused_max{-1};

int rt_debug_set_bloom_fused(int32_t max_stride) {
    return g_bloom_fused_max.exchange(max_stride < 0 ? -1 : max_stride > BLOOM_FUSED_MAX_STRIDE ? BLOOM_FUSED_MAX_STRIDE : max_stride);
}

int rt_bloom_params_init_sized(rt_bloom_params *params, uint32_t struct_size) {
    return params_init_sized(params, struct_size, "rt_bloom_params_init_sized", rtbl::size_known, rtbl::defaults);
}

int64_t rt_bloom_workspace_bytes(int32_t width, int32_t height) { return rtbl::workspace_bytes(width, height); }

int rt_bloom_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const rt_bloom_params *params,
                    double *d_mean_out, void *d_workspace, void *hip_stream) {
    const std::string w("rt_bloom_device");
    rt_bloom_params p;
    if (const char *bad = rtbl::bad_argument(true, width, height, d_values, d_mean_out, d_workspace, spp, params, p))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    if (((uintptr_t)d_workspace & 15u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    const size_t n_pix = (size_t)width * (size_t)height, frame_bytes = n_pix * 3u * sizeof(double);
    if (overlaps(d_mean_out, frame_bytes, d_values, frame_bytes)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_mean_out must not overlap d_values");
    if (int rc = select_device_of(d_mean_out, "rt_bloom_device")) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t region = rtbl::region_bytes(width, height);
    // the three regions: `cur` holds B_k, `other` takes H (two passes: V writes B_k+1 back into cur) or B_k+1 itself (one launch: they swap)
    double *cur = (double *)d_workspace, *other = (double *)((char *)d_workspace + region), *a = (double *)((char *)d_workspace + 2 * region);
    const double inv_spp = 1.0 / (double)spp;
    launch_bloom_bright((int64_t)n_pix, d_values, inv_spp, d_spp, p.threshold, cur, a, stream);
    HIP_TRY(hipGetLastError());
    const BloomOutput out{d_values, inv_spp, d_spp, p.levels, p.strength, d_mean_out};
    int32_t fused_max = g_bloom_fused_max.load();
    if (fused_max < 0) fused_max = bloom_fused_tiles(width, height) >= BLOOM_FUSED_MIN_TILES ? BLOOM_FUSED_MAX_STRIDE : 0;
    for (int32_t k = 0; k < p.levels; ++k) {
        const int32_t stride = 1 << k;
        const BloomOutput *last = k == p.levels - 1 ? &out : nullptr;
        if (stride <= fused_max) {
            launch_bloom_level_fused(width, height, stride, cur, other, a, last, stream);
            HIP_TRY(hipGetLastError());
            std::swap(cur, other);
        } else {
            launch_bloom_h(width, height, stride, cur, other, stream);
            HIP_TRY(hipGetLastError());
            launch_bloom_v(width, height, stride, other, cur, a, last, stream);
            HIP_TRY(hipGetLastError());
        }
    }
    return RT_OK;
}

// ---- robust frames (rt_robust.hip): K block means per value, combined by a trimmed mean of their sorted order ----

// The kernel form: the slots of its sorting network; 0: the built-in rule, the smallest form that fits (rt_debug_set_robust_form; speed only).
static std::atomic<int32_t> g_robust_form{0};

int rt_debug_set_robust_form(int32_t slots) {
    return g_robust_form.exchange(slots <= 0 ? 0 : rtrb::kmax_for(slots > RT_ROBUST_MAX_BLOCKS ? RT_ROBUST_MAX_BLOCKS : slots));
}

int rt_robust_params_init_sized(rt_robust_params *params, uint32_t struct_size) {
    if (!params) return fail(RT_ERR_INVALID_ARGUMENT, "rt_robust_params_init_sized: null argument");
    if (!rtrb::size_known(struct_size)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_robust_params_init_sized: struct_size is not one this library knows");
    rt_robust_params full;
    rtrb::defaults(full);
    full.struct_size = struct_size;
    memcpy(params, &full, struct_size);
    return RT_OK;
}

int rt_robust_device(int32_t width, int32_t height, int32_t blocks, const double *d_stack, int32_t spp, const rt_robust_params *params,
                     double *d_mean_out, double *d_m2_out, void *hip_stream) {
    const std::string w("rt_robust_device");
    rt_robust_params p;
    if (const char *bad = rtrb::bad_argument(true, width, height, blocks, d_stack, d_mean_out, spp, params, p))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    if (const char *bad = rtrb::bad_overlap(true, width, height, blocks, d_stack, d_mean_out, d_m2_out)) return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    if (int rc = select_device_of(d_mean_out, "rt_robust_device")) return rc;
    launch_robust(g_robust_form.load(), 3 * (int64_t)width * height, d_stack, blocks, p.mode, p.trim, p.gain, 1.0 / (double)spp, d_mean_out, d_m2_out,
                  (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- guided upsampling (rt_upsample.hip): a small beauty frame brought to full size under full-size albedo and surface-ID guides ----

int rt_camera_scaled(const rt_camera *camera, int32_t factor, rt_camera *out) {
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_scaled: camera is null");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_scaled: out is null");
    if (!rtup::factor_ok(factor)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_scaled: factor must be 2, 3 or 4");
    rt_camera c = *camera;
    const double f = (double)factor;
    c.image_width = rtm::rt_up_low_size(camera->image_width, factor);
    c.image_height = rtm::rt_up_low_size(camera->image_height, factor);
    // per component: du' = F * du; dv' = F * dv; p00' = (p00 - (0.5 * (du + dv))) + (0.5 * (du' + dv'))
    auto scale = [&](double p00, double du, double dv, double &p00_out, double &du_out, double &dv_out) {
        const double du2 = f * du, dv2 = f * dv;
        const double corner = p00 - (0.5 * (du + dv));
        p00_out = corner + (0.5 * (du2 + dv2));
        du_out = du2;
        dv_out = dv2;
    };
    scale(camera->pixel00_loc.x, camera->pixel_delta_u.x, camera->pixel_delta_v.x, c.pixel00_loc.x, c.pixel_delta_u.x, c.pixel_delta_v.x);
    scale(camera->pixel00_loc.y, camera->pixel_delta_u.y, camera->pixel_delta_v.y, c.pixel00_loc.y, c.pixel_delta_u.y, c.pixel_delta_v.y);
    scale(camera->pixel00_loc.z, camera->pixel_delta_u.z, camera->pixel_delta_v.z, c.pixel00_loc.z, c.pixel_delta_u.z, c.pixel_delta_v.z);
    *out = c;
    return RT_OK;
}

// Which form rt_upsample_device launches: 0 the direct one, 1 the LDS one; negative: the built-in rule (rt_debug_set_upsample_form; speed
// only).  The rule is DESIGN.md "Upsampling"'s measurement: the LDS form always — it is 9 - 24 % ahead at 1200 x 800 (3800 tiles) and
// 5 - 22 % ahead at 256 x 256 (256 tiles), with every guide set.
static std::atomic<int32_t> g_upsample_form{-1};

int rt_debug_set_upsample_form(int32_t form) { return g_upsample_form.exchange(form < 0 ? -1 : form > 0 ? 1 : 0); }

int rt_upsample_params_init_sized(rt_upsample_params *params, uint32_t struct_size) {
    return params_init_sized(params, struct_size, "rt_upsample_params_init_sized", rtup::size_known, rtup::defaults);
}

int64_t rt_upsample_workspace_bytes(int32_t width, int32_t height, int32_t factor) { return rtup::workspace_bytes(width, height, factor); }

int rt_upsample_device(int32_t width, int32_t height, const double *d_low, int32_t spp, const double *d_albedo_sum, int32_t albedo_spp,
                       const double *d_edge_sum, int32_t edge_spp, const rt_upsample_params *params, double *d_mean_out, uint8_t *d_rgba8,
                       void *d_workspace, void *hip_stream) {
    const std::string w("rt_upsample_device");
    rt_upsample_params p;
    if (const char *bad = rtup::bad_argument(true, width, height, d_low, d_mean_out, d_workspace, spp, d_albedo_sum, albedo_spp, d_edge_sum, edge_spp,
                                             params, p))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    if (((uintptr_t)d_rgba8 & 3u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_rgba8 must be 4-byte aligned");
    if (((uintptr_t)d_workspace & 15u) != 0) return fail(RT_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    if (const char *bad = rtup::bad_overlap(true, width, height, p.factor, d_mean_out, d_low, d_albedo_sum, d_edge_sum))
        return fail(RT_ERR_INVALID_ARGUMENT, w + ": " + bad);
    if (int rc = select_device_of(d_mean_out, "rt_upsample_device")) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t region = rtup::region_bytes(width, height, p.factor);
    UpsampleArgs u{};
    u.w = width; u.h = height; u.lw = rtm::rt_up_low_size(width, p.factor); u.lh = rtm::rt_up_low_size(height, p.factor); u.factor = p.factor;
    u.low = d_low; u.inv_spp = 1.0 / (double)spp;
    u.albedo_sum = d_albedo_sum; u.n_a = (double)albedo_spp;
    u.edge_sum = d_edge_sum; u.n_e = (double)edge_spp;
    u.sigma_albedo = p.sigma_albedo; u.sigma_edge = p.sigma_edge; u.albedo_floor = p.albedo_floor;
    u.rec_r = (double *)d_workspace; u.rec_a = (double *)((char *)d_workspace + region); u.rec_g = (double *)((char *)d_workspace + 2 * region);
    u.out = d_mean_out; u.rgba = (uint32_t *)d_rgba8;
    launch_upsample_prepare(u, stream);
    HIP_TRY(hipGetLastError());
    const int32_t form = g_upsample_form.load();
    launch_upsample(u, form != 0, stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- panoramas (rt_panorama.hip): six cube-face cameras, the longitude and latitude tables, and the cube-to-equirectangular resampler ----

int rt_camera_cube_faces(const rt_camera *like, const double center[3], int32_t face_size, int32_t guard, rt_camera out[6]) {
    if (!like) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_cube_faces: like is null");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_camera_cube_faces: out is null");
    if (const char *bad = rtpn::bad_face(face_size, guard)) return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_camera_cube_faces: ") + bad);
    rtpn::cube_faces(*like, center, face_size, guard, out);
    return RT_OK;
}

int rt_panorama_tables(int32_t width, int32_t height, double *tables) {
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_panorama_tables: width and height must be positive");
    if ((int64_t)width * height >= rtpn::MAX_PIXELS) return fail(RT_ERR_INVALID_ARGUMENT, "rt_panorama_tables: width x height must be below 2^27 pixels");
    if (!tables) return fail(RT_ERR_INVALID_ARGUMENT, "rt_panorama_tables: tables is null");
    rtpn::tables(width, height, tables);
    return RT_OK;
}

int rt_panorama_device(int32_t width, int32_t height, const double *d_tables, const double *d_faces, int32_t face_size, int32_t guard, int32_t spp,
                       double *d_mean_out, void *hip_stream) {
    if (const char *bad = rtpn::bad_argument(true, width, height, d_tables, d_faces, face_size, guard, spp, d_mean_out))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_panorama_device: ") + bad);
    if (int rc = select_device_of(d_mean_out, "rt_panorama_device")) return rc;
    launch_panorama(width, height, d_tables, d_faces, face_size, guard, 1.0 / (double)spp, d_mean_out, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- frame metrics (rt_metrics.hip): a frame's error against a reference and its own noise estimate, each one tree reduction ----

int rt_frame_error_params_init_sized(rt_frame_error_params *params, uint32_t struct_size) {
    return params_init_sized<rt_frame_error_params>(params, struct_size, "rt_frame_error_params_init_sized", rtmt::error_size_known, rtmt::defaults);
}

int rt_frame_noise_params_init_sized(rt_frame_noise_params *params, uint32_t struct_size) {
    return params_init_sized<rt_frame_noise_params>(params, struct_size, "rt_frame_noise_params_init_sized", rtmt::noise_size_known, rtmt::defaults);
}

int64_t rt_metrics_workspace_bytes(int32_t width, int32_t height) { return rtmt::workspace_bytes(width, height); }

int rt_frame_error_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const double *d_ref, int32_t ref_spp,
                          const rt_frame_error_params *params, double *d_out8, void *d_workspace, void *hip_stream) {
    rt_frame_error_params p;
    if (const char *bad = rtmt::bad_error_argument(true, width, height, d_values, spp, d_ref, ref_spp, params, d_out8, d_workspace, p))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_frame_error_device: ") + bad);
    if (int rc = select_device_of(d_out8, "rt_frame_error_device")) return rc;
    launch_frame_error((int64_t)width * height, d_values, 1.0 / (double)spp, d_spp, d_ref, 1.0 / (double)ref_spp, p.eps, p.peak, (double *)d_workspace,
                       d_out8, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_frame_noise_device(int32_t width, int32_t height, int32_t form, const double *d_a, const double *d_b, int32_t n, const int32_t *d_spp,
                          const rt_frame_noise_params *params, double *d_out4, void *d_workspace, void *hip_stream) {
    rt_frame_noise_params p;
    if (const char *bad = rtmt::bad_noise_argument(true, width, height, form, d_a, d_b, n, d_spp, params, d_out4, d_workspace, p))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_frame_noise_device: ") + bad);
    if (int rc = select_device_of(d_out4, "rt_frame_noise_device")) return rc;
    launch_frame_noise((int64_t)width * height, form == RT_METRICS_MEANS, d_a, d_b, n, d_spp, p.eps, (double *)d_workspace, d_out4, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_resolve_rgb8_spp_device(int32_t width, int32_t height, const double *d_sum, const int32_t *d_spp, uint8_t *d_rgb8, void *hip_stream) {
    if (!d_sum || !d_spp || !d_rgb8 || width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_resolve_rgb8_spp_device: bad argument");
    if (int rc = select_device_of(d_rgb8, "rt_resolve_rgb8_spp_device")) return rc;
    launch_resolve_rgb8_spp((int64_t)width * height, d_sum, d_spp, d_rgb8, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

} // extern "C"
