// rt_kernels.h — the seam between the device code (rt_kernel.hip) and the host side of librt_amd (rt_api.cpp, rt_debug.cpp):
// the kernels' parameter block, the feature bits a kernel instantiation is compiled for, and the launch entry points.
#pragma once
#include "rt_amd.h"
#include "rt_layout.h"

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <cstdint>
#include <initializer_list>

namespace rtk {
using namespace rtd;

struct DMaterial { // 64 bytes
    uint32_t kind;
    uint32_t texture;
    uint32_t needs_uv; // the texture below reads (u, v): only ImageTexture does (src/texture.rs:83)
    uint32_t solid;    // the texture is a SolidColor: its colour is copied into `albedo` (one dependent load fewer per hit)
    double albedo[3];  // Metal's albedo, or the SolidColor's colour; a Dielectric's 1 / ir, r0 seen from outside, r0 seen from inside (rt_api.cpp)
    double fuzz;
    double ir;
    uint32_t slow;     // evaluating the texture is dear (Perlin turbulence): see the shade stage
    uint32_t _pad2;
};
static_assert(sizeof(DMaterial) == 64, "DMaterial must be 64 bytes");

// What a "local tile" of a render's job space is (path_kernel's JOBS): a tile of the frame; a group of 64 entries of a pixel list
// (rt_render_pixels_device); a tile of one of several views of the scene, view v's tiles behind view v - 1's (rt_render_views_device)
enum JobMode : int { JOBS_DENSE = 0, JOBS_LIST = 1, JOBS_VIEWS = 2 };

// views mode: what a lane needs of its job's view, one record per view (lanes of one wave sit in different views, so the record is read
// from global memory per lane: 16-byte aligned and padded, for the widest vector loads)
struct alignas(16) ViewRec {
    rt_camera cam;
    uint64_t seed_mixed; // mix64(seed + gamma) of the view's seed
    uint64_t _pad;
};
static_assert(sizeof(ViewRec) == 208 && sizeof(ViewRec) % 16 == 0, "ViewRec: a whole number of 16-byte pieces");

struct KParams {
    const Node32 *nodes;
    const Sphere *spheres;
    const Quad *quads;
    const Instance *insts;
    const Medium *media;
    const DMaterial *mats;
    const rt_texture *texs;
    const rt_perlin *perlins;
    const ImageRef *images;
    const uint8_t *texels;
    const double *srgb_lut;
    double *out;
    double *samples;                // [local tile][sample of this launch][64 pixels][3]: one colour per camera path
    double *att_stack;              // [max_depth + 1][3][n_threads]: parked attenuations that are a texture's value
    uint32_t *att_ids;              // [max_depth + 1 - 8][n_threads]: parked material indices that no longer fit the lane's registers
    uint32_t ids_ok;                // 1: material indices fit 16 bits (else every attenuation is parked as a colour, by a kernel with textures)
    uint32_t id_one;                // index of the material table's extra last entry, whose albedo is Color::ONE
    uint32_t *job_counter;
    unsigned long long *counters;   // rt_counters as 10 u64, then per profile slot (9): rounds, active lanes, cycles; or null
    rt_camera cam;
    uint64_t seed_mixed;            // mix64(seed + gamma)
    uint32_t n_nodes;
    uint32_t n_threads;
    int32_t sample_begin;           // first sample of this launch
    uint32_t n_samples;             // samples per pixel in this launch
    uint32_t n_jobs;                // n_local_tiles * n_samples * 64
    uint32_t jobs_per_grab;
    float grab_taper;               // a grab takes at most this fraction of the jobs still to hand out (guided self-scheduling)
    double inv_n_samples, inv_tiles_x; // 1 / n_samples, 1 / tiles_x (job decode)
    int32_t max_depth, accumulate;
    int32_t shard_index, shard_count, out_layout;
    int32_t tiles_x;
    uint32_t n_local_tiles;
    uint32_t th_prim, th_other, th_shade, th_new; // scheduler thresholds, in 64ths of the live lanes
    uint32_t th_box;                // the box loop keeps running while this many 64ths of the live lanes are in it
    uint32_t th_pack;               // path_kernel reads the four above from here: prim | other << 8 | shade << 16 | box << 24 (each <= 255)
    uint32_t defer_instances;       // ordered walk: 1 = the world frame's Translate/RotateY subtrees are walked after the world's own tree (path_kernel)
    // LDS-resident scene (SCENE_IN_LDS kernels): image to copy in, and where its parts start (bytes)
    const uint4 *lds_image;
    uint32_t lds_image_bytes;
    uint32_t lds_off_node_b, lds_off_spheres, lds_off_quads;
    uint32_t lds_off_qfilt;         // the quads' f32 filter records (rt_layout.h QFiltPair), behind the quads; 0xffffffff: none, every quad gets the exact test
    double *world_slots;            // [6][n_threads] doubles: a lane's world-frame ray while it walks inside a frame
    uint32_t lds_world_off;         // ... or, where the LDS has room, [6][block threads] doubles there (0xffffffff: global memory)
    // ordered layout (rt_layout.h): records, the world frame's root, and where the per-lane stacks start in the LDS
    const uint4 *oimage;            // the seven tables of load_opair, in global memory (LDS kernels copy them in)
    const OSeq *oseq;               // the world frame's sequence of trees and media (rt_layout.h)
    float box_extent;               // the largest |coordinate| of any box of the ordered layout (box_pair_f32's B)
    const uint4 *aux_image;         // AUX kernels: materials | textures | frames | media | Perlin tables, to copy into the LDS
    uint32_t aux_bytes, lds_aux_off, aux_off_mats, aux_off_texs, aux_off_insts, aux_off_media, aux_off_perlins;
    uint32_t n_oseq;
    uint32_t o_root;
    // a query may start with the primitives of a leaf under the root instead of the root record (rt_api.cpp "start shortcut"): the stage of the
    // leaf's kind (ST_SPHERE / ST_QUAD; 0: no shortcut), its primitives [prim, end), the root's other child, which child of the root the leaf is
    // (wide records: o_start_rest is the stack entry itself, in the launch's format — the root with the mask of its children NOT to look at, or the
    // one other child's own entry, its index, if that is an inner record (setaside_direct); all ones: nothing to set aside)
    uint32_t o_start_stage, o_start_prim, o_start_end, o_start_rest, o_start_slot;
    uint32_t setaside_direct;       // wide records: 1 = a record with one child left to look at sets that child aside itself if it is an inner record (RT_WIDE_SETASIDE)
    uint32_t inst_shortcut;         // 1: a walk that enters a frame whose tree is one leaf starts with the leaf's primitives (Instance::start_ref)
    uint32_t slow_min, slow_age;    // shade stage: lanes with a dear texture wait for this many of their kind, at most this many shade rounds
    uint32_t medium_first;          // 1: the draw of a sphere-bounded medium the ray starts inside is made before the tree in front of it is walked (path_kernel)
    uint32_t seq_lookahead;         // 1: a query that cannot reach any later step of the world's sequence ends it at its start (path_kernel)
    uint32_t lds_stack_off;
    uint32_t lds_seq_off;           // the world frame's sequence, copied in by the ordered kernels (after the stacks)
    uint32_t lds_prof_off;          // COUNT kernels: per-wave profile rows (last)
    // 1: the start shortcut's leaf is ONE sphere and its test runs where the query starts, for the lanes that start one, not in a round of
    // the sphere stage (path_kernel "inline start test"; RT_START_INLINE).  (The word sits in what was padding: no other argument moves.)
    // A kernel may IGNORE it: only the spheres-only ordered kernels (FEAT_SPHERES_SOLID) have the test compiled in; in every other one — a
    // textured scene with a ground sphere runs the textures kernel — the leaf is tested in the sphere stage as before, the word set or not
    // (rt_debug_last_start reports the word, rt_debug_last_kernel the kernel).
    uint32_t start_inline;
    // list mode (rt_render_pixels_device; path_kernel<..., LIST = true>): a "local tile" is a group of 64 entries of this list instead;
    // an entry that is no pixel of the frame (0xffffffff: padding) traces nothing.  The dense instantiations never read these four.
    const uint32_t *pixel_list;
    uint32_t n_list;                // entries of pixel_list (the groups beyond it are padding)
    double inv_width;               // 1 / image_width (list mode's pixel -> (i, j) decode; exact for w * h < 2^27)
    double *out_sq;                 // the reduction's second moments beside `out`, laid out as `out` is (launch_reduce_samples): sums of the
                                    // squared sample colours (list mode: or null; views with moments) or Welford's running M2 (mean with moments)
    // views mode (rt_render_views_device; path_kernel<..., JOBS_VIEWS>): local tile lt is tile lt % tiles_per_view of view lt / tiles_per_view.
    // `cam` then holds what the views share (frame size); camera and seed of a job come from its view's record.  No other instantiation reads these.
    const ViewRec *views;
    double inv_tiles_per_view;      // 1 / tiles_per_view (exact decode for lt < 2^27)
    uint32_t tiles_per_view;
    // live refinement (rt_render_mean_device; the reduction's mean folds): `out` is the frame of running means and `sample_begin` the
    // number of samples already in it; the display frame (4 bytes per pixel, 4-byte aligned) that the last launch of a call writes, or null.
    // No other kernel reads this.
    uint8_t *mean_rgba8;
};

// What a scene can contain.  A kernel instantiated without a feature has that code compiled out, which matters for
// more than its size: the register allocation of the whole kernel is set by its hungriest path.
enum Feature : uint32_t {
    F_SPHERES = 1u,  // Sphere leaves
    F_QUADS = 2u,    // Quad leaves
    F_FRAMES = 4u,   // Translate / RotateY
    F_MEDIA = 8u,    // ConstantMedium
    F_TEXTURES = 16u // Checker / Image / Noise textures (without it every texture is a SolidColor)
};
constexpr uint32_t F_ALL = 31u;

constexpr uint32_t PROF_SLOTS = 12;      // COUNT kernels: profile slots per wave (6 stages + 6 parts of the shade / path-end rounds)
// COUNT kernels, wide records: visits by kind (rt_amd_debug.h rt_debug_visit_stats): [0] first visits of a record; [1 + 3 (b - 1) + o]
// revisits of a record set aside with b children still to look at (b = 1..3), o = what the lane went on with: 0 an inner record,
// 1 a leaf or an instance, 2 nothing (every child culled); [10] entries set aside as a record with a mask, [11] as a child's own entry
constexpr uint32_t VISIT_STATS = 12;
constexpr uint32_t COUNTER_WORDS = 10 + PROF_SLOTS * 3 + VISIT_STATS; // rt_counters as 10 u64, then per profile slot: rounds, active lanes, cycles, then VISIT_STATS
// Jobs a wave reserves at a time: a multiple of 64 (one sample-row of an 8x8 tile, so the lanes a wave starts together
// trace neighbouring pixels).  Large grabs mean few atomics; small ones a short tail (the last grab of the slowest wave
// is all that is left running at the end): launch_render picks the size so that every wave gets at least ~32 grabs.
// (one device counter serves every wave: reservations have to stay well under ~88 per microsecond machine-wide)
constexpr uint32_t MAX_JOBS_PER_GRAB = 1024, MIN_JOBS_PER_GRAB = 128, MIN_JOBS_PER_WAVE = 256;

constexpr int GLOBAL_THREADS = 256;             // scene gathered from global memory: 256-thread blocks
#ifndef RT_LDS_THREADS
#define RT_LDS_THREADS 1024 // 16 waves = 4 per SIMD (tools/tune.py: 512 -> 1381, 768 -> 1774, 1024 -> 1921 Msamples/s on C2 at 48 spp)
#endif
constexpr int LDS_THREADS = RT_LDS_THREADS;     // scene in LDS: one 16-wave workgroup per CU shares the copy
#ifndef RT_LDS_THREADS_GENERAL
#define RT_LDS_THREADS_GENERAL 1024 // the every-feature kernels: 16 waves = 4 per SIMD at 128 registers.  (Rounds 1-2: 768 threads, 3 per SIMD at 168 registers —
// at 128 they spilled 80-141 of them; with the parked indices, the parameters and the slot addresses read at use they spill 0-75, nearly all of it in cold
// code, and the fourth wave pays: cornell_smoke 1296 -> 1465 Msamples/s, two_perlin_spheres 4663 -> 5082, simple_light 5684 -> 5871; the reference-order texture kernel is the exception, below)
#endif
constexpr int LDS_THREADS_GENERAL = RT_LDS_THREADS_GENERAL;
#ifndef RT_QUADS_FRAMES_THREADS
#define RT_QUADS_FRAMES_THREADS RT_LDS_THREADS // the quads + frames kernel (Cornell): 128 registers with 6-10 spilled at 1024 threads; tools A/B: 768
#endif
constexpr int QUADS_FRAMES_THREADS = RT_QUADS_FRAMES_THREADS;
// spheres + quads + textures in the REFERENCE's order (earth, a one-sphere scene, renders that way by default; the fallback of two_spheres,
// two_perlin_spheres, simple_light): 12 waves = 3 per SIMD at 168 registers.  At 1024 threads that kernel spills 48 registers in its
// texture code, which a one-primitive scene runs all the time: earth 17.6 Gsamples/s at 1024 threads, 22.1 at 768 (256 spp; the other
// three in reference order 5.6 / 2.9 / 5.6 -> 6.7 / 3.2 / 6.0).  The same features on the library's own trees keep 1024 (8.3 / 5.1 / 7.7
// against 8.1 / 4.8 / 7.3 at 768), and so does every kernel with media (cornell_smoke 1.50 against 1.32; reference order 1.17 / 1.03).
constexpr int REFERENCE_TEXTURES_THREADS = 768;
constexpr size_t LDS_BUDGET_BYTES = 160 * 1024; // LDS per CU on MI355X

// The kernel instantiations that exist: the general one (every feature) at each LDS level, plus specialised
// ones for scenes that fit the LDS entirely and use a subset of the features (BASELINE configs 1/2 and 3).
constexpr uint32_t FEAT_SPHERES_SOLID = F_SPHERES;          // random-spheres: spheres, solid colours
constexpr uint32_t FEAT_QUADS_FRAMES = F_QUADS | F_FRAMES;  // Cornell box: quads, cubes in Translate/RotateY frames
// two more, at 768 threads (3 waves per SIMD), which need no spill there: 156 and 150 registers (the every-feature kernel: 168 + 16..38 spilled)
constexpr uint32_t FEAT_QUADS_FRAMES_MEDIA = F_QUADS | F_FRAMES | F_MEDIA;              // cornell_smoke
constexpr uint32_t FEAT_SPHERES_QUADS_TEXTURES = F_SPHERES | F_QUADS | F_TEXTURES;    // two_spheres, earth, two_perlin_spheres, simple_light
inline uint32_t kernel_features_for(uint32_t scene_features, int lds, bool ordered) {
    (void)ordered;
    if (lds == 3) { // the specialised instantiations exist for scenes that live in the LDS whole
        for (uint32_t f : {FEAT_SPHERES_SOLID, FEAT_QUADS_FRAMES, FEAT_QUADS_FRAMES_MEDIA, FEAT_SPHERES_QUADS_TEXTURES})
            if ((scene_features & ~f) == 0) return f;
    }
    return F_ALL;
}
inline int kernel_threads_for(uint32_t kernel_features, int lds, bool ordered) { // workgroup size of that instantiation
    if (lds == 0) return GLOBAL_THREADS;
    if (kernel_features == FEAT_QUADS_FRAMES) return QUADS_FRAMES_THREADS;
    if (kernel_features == FEAT_SPHERES_QUADS_TEXTURES && !ordered) return REFERENCE_TEXTURES_THREADS;
    return kernel_features == FEAT_SPHERES_SOLID ? LDS_THREADS : LDS_THREADS_GENERAL;
}
const void *path_kernel_for(int lds, bool counted, uint32_t feat, bool ordered, bool aux, bool wide, int jobs = JOBS_DENSE);

// launches of the small kernels (all asynchronous on `stream`; errors through hipGetLastError)
// the per-pixel reduction of a launch's sample buffer into K.out (rt_kernel.hip reduce_samples), one kernel per route: the sum (dense
// jobs; a pixel list; views), the sum with each view's sums of squares in K.out_sq, the running mean, the mean with Welford's M2 in K.out_sq
enum class Reduce { Sum, Listed, Views, ViewsMoments, Mean, MeanMoments };
void launch_reduce_samples(Reduce r, const KParams &K, unsigned grid, hipStream_t stream); // (grid blocks of 256 threads)
// adaptive sampling (rt_render_adaptive_device): the list of every pixel in tile order; one convergence step over an active list
// (spp of the pixels that leave, the survivors compacted in order into list_out, padded to a multiple of 64, their count in *count);
// the resolve with a per-pixel sample count
void launch_tile_order_list(int32_t w, int32_t h, uint32_t *list, hipStream_t stream);
struct AdaptiveScratch {
    unsigned long long *masks; // one ballot of survivors per wave of the step
    uint32_t *block_base;      // survivors per block, then (scanned) the block's offset in list_out
    uint32_t *count;           // survivors
};
void launch_adaptive_step(const uint32_t *list_in, uint32_t n_in, uint32_t n_pixels, const double *sum, const double *sum_sq, int32_t n,
                          int32_t last, double rel, double abs, int32_t *spp, uint32_t *list_out, const AdaptiveScratch &x, hipStream_t stream);
void launch_resolve_rgb8_spp(int64_t n_pixels, const double *sum, const int32_t *spp, uint8_t *rgb, hipStream_t stream);
void launch_tiles_to_frame(int32_t w, int32_t h, int32_t tiles_x, int32_t shard_count, int64_t shard_stride, const double *gathered,
                           double *frame, hipStream_t stream);
void launch_tiles_to_frame_rgb8(int32_t w, int32_t h, int32_t tiles_x, int32_t shard_count, int64_t shard_stride, const uint8_t *gathered,
                                uint8_t *frame, hipStream_t stream);
void launch_resolve_rgb8(int64_t n_values, double inv_spp, const double *sum, uint8_t *rgb, hipStream_t stream);
void launch_resolve_rgba8(int64_t n_pixels, const double *mean, uint8_t *rgba, hipStream_t stream);
// the denoisers (rt_denoise.hip; rt_denoise_device and, with a guide, rt_denoise_albedo_device): `half` / `half_in` / `half_out` are
// halves of the caller's workspace, one double4 (C_r, C_g, C_b, V) per pixel.  `guide` null is the plain filter; otherwise the albedo
// frame and the guided filter's two parameters, and `region`, a third region of the workspace of one double4 (a_r, a_g, a_b, 0) per
// pixel that prepare writes once and the iterations read.  An iteration with half_out null is the last: it writes mean_out (3 w h
// doubles; guided: with the floored albedo multiplied back in) and, if not null, rgba8.  `means`: the inputs are a frame of running
// means and of M2 after `spp` samples of every pixel (rt_denoise_mean_device; no spp map), and the guide's frame holds means as well.
// `n_views` (1..65535: the grid's second dimension) frames are filtered by one launch: every buffer — the inputs, each half, the guide's
// frame and its region, mean_out, rgba8 — then holds n_views frames one behind the other, and no tap leaves its own frame.  1 is the
// single frame.  (The spatial prepare has no views form.)
struct DenoiseGuide {
    const double *albedo_sum; // 3 w h doubles: per-pixel sums of albedo_spp samples (prepare reads them); means form: their means
    double albedo_spp;        // their count, as the divisor it is (means form: not read)
    double albedo_floor, sigma_albedo;
    double4 *region;
};
// the edge guide (rt_denoise_guided_device and its means, spatial and views forms): a frame that contributes one stop factor per tap and nothing
// else.  `edge` null: none.  Alone it takes the albedo guide's place in the workspace (the third region) and in the staged planes;
// beside an albedo guide its region of one double4 (g_r, g_g, g_b, 0) per pixel is a fourth.
struct DenoiseEdge {
    const double *edge_sum; // 3 w h doubles: per-pixel sums of edge_spp samples of the guide frame (prepare reads them); means form: their means
    double edge_spp;        // their count, as the divisor it is (means form: not read)
    double sigma_edge;
    double4 *region;
};
void launch_denoise_prepare(int64_t n_pixels /* of one frame */, int32_t n_views, const double *sum, const double *sum_sq, int32_t spp, const int32_t *spp_map, const DenoiseGuide *guide,
                            bool means, void *half, hipStream_t stream, const DenoiseEdge *edge = nullptr);
// the spatial prepare (rt_denoise_mean_spatial_device below its threshold) in launch_denoise_prepare's place: `mean` and, guided,
// guide->albedo_sum are frames of means; V0 is the spread of C0 over the (2 radius + 1)^2 window, radius 1..3.  With `edge`
// (edge->edge_sum: a frame of means as well) the window holds only the pixels the edge stop lets through from its centre
void launch_denoise_prepare_spatial(int32_t w, int32_t h, int32_t radius, const double *mean, const DenoiseGuide *guide, void *half, hipStream_t stream,
                                    const DenoiseEdge *edge = nullptr);
void launch_denoise_atrous(int32_t w, int32_t h, int32_t n_views, int32_t stride, double sigma, double eps, const DenoiseGuide *guide, const void *half_in,
                           void *half_out, double *mean_out, uint8_t *rgba8, hipStream_t stream, const DenoiseEdge *edge = nullptr);
// the tone-mapping stage (rt_tonemap.hip; rt_tonemap_device, rt_log_average_luminance_device).  launch_log_average runs every level of
// the log-average tree over a frame of n_pixels pixels (values: 3 per pixel; a pixel's mean is its value times inv_spp or, with a
// map, times 1 / spp_map[pixel]): `partials` has room for the blocks of every level, level 0's first (rt_tonemap_workspace_bytes), and
// the last level writes log_mean, Lavg, count and — auto_key > 0 — scale = exposure * (auto_key / Lavg), else 0, to out4.  The value
// kernels read the scale from d_scale if it is not null (device memory: out4 + 3), else take `scale`; w2 = white * white.
struct TonemapPartial { double t; uint64_t count; };
static_assert(sizeof(TonemapPartial) == 16, "TonemapPartial: 16 bytes per block of the workspace");
void launch_log_average(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double delta, TonemapPartial *partials,
                        double exposure, double auto_key, double *out4, hipStream_t stream);
void launch_tonemap_rgb8(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale, int32_t op,
                         double w2, uint8_t *rgb, hipStream_t stream);
void launch_tonemap_rgba8(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale, int32_t op,
                          double w2, uint8_t *rgba, hipStream_t stream);
// the film stage (rt_film.hip; rt_film_device): the tone-mapping value kernels' arguments, and `out` in the layout of `format`
// (RT_FILM_RGBE: n_pixels words; RT_FILM_F32: 3 n_pixels floats; RT_FILM_RGB16: 3 n_pixels uint16)
void launch_film(int32_t format, int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double scale, const double *d_scale,
                 int32_t op, double w2, void *out, hipStream_t stream);
// bloom (rt_bloom.hip; rt_bloom_device).  Frames are 3 doubles per pixel, row after row.  launch_bloom_bright writes every pixel's B0
// to b0 and +0.0 to a.  A level at `stride` reads b_in and leaves B_k+1 in b_out and A += B_k+1 in a; on the last level it writes
// out = m + strength * (A / levels) instead, from values / inv_spp / spp_map, and neither b_out nor a.  launch_bloom_level_fused is
// the level as one launch (stride 1 or 2 — BLOOM_FUSED_MAX_STRIDE; b_out must not be b_in), one workgroup per tile of 64 x 16 pixels,
// bloom_fused_tiles of them; launch_bloom_h and launch_bloom_v are its two global passes at any stride (h: b_in -> h_out; v: h_in ->
// b_out, which may be the b_in of the h pass).
constexpr int32_t BLOOM_FUSED_MAX_STRIDE = 2;
int64_t bloom_fused_tiles(int32_t w, int32_t h);
struct BloomOutput { const double *values; double inv_spp; const int32_t *spp_map; int32_t levels; double strength; double *out; };
void launch_bloom_bright(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, double threshold, double *b0, double *a,
                         hipStream_t stream);
void launch_bloom_level_fused(int32_t w, int32_t h, int32_t stride, const double *b_in, double *b_out, double *a, const BloomOutput *last,
                              hipStream_t stream);
void launch_bloom_h(int32_t w, int32_t h, int32_t stride, const double *b_in, double *h_out, hipStream_t stream);
void launch_bloom_v(int32_t w, int32_t h, int32_t stride, const double *h_in, double *b_out, double *a, const BloomOutput *last, hipStream_t stream);
// robust frames (rt_robust.hip; rt_robust_device).  One launch, one thread per value of the 3 w h (`total`): `blocks` frames of `total`
// doubles at `stack`, block after block, into mean_out and, if not null, m2_out.  kmax picks the kernel form — 4, 8, 16 or 32 register
// slots; one too small for `blocks` counts as the smallest that fits (what rt_api.cpp passes by itself) — and changes no bit.
void launch_robust(int32_t kmax, int64_t total, const double *stack, int32_t blocks, int32_t mode, int32_t trim, double gain, double inv_spp,
                   double *mean_out, double *m2_out, hipStream_t stream);
// guided upsampling (rt_upsample.hip; rt_upsample_device).  w x h is the FULL size, lw x lh the low one; rec_r, rec_a and rec_g are the
// workspace's regions of 4 doubles per low pixel (rt_upsample_shared.h).  launch_upsample_prepare writes rec_r and, per guide given
// (albedo_sum / edge_sum not null), rec_a / rec_g; launch_upsample reads them and writes out (3 w h doubles) and, if not null, rgba (w h
// words): lds = true stages a tile's records in the LDS, false reads every tap from the regions; the bits are the same.
struct UpsampleArgs {
    int32_t w, h, lw, lh, factor;
    const double *low; double inv_spp;
    const double *albedo_sum; double n_a;
    const double *edge_sum; double n_e;
    double sigma_albedo, sigma_edge, albedo_floor;
    double *rec_r, *rec_a, *rec_g;
    double *out; uint32_t *rgba;
};
void launch_upsample_prepare(const UpsampleArgs &u, hipStream_t stream);
void launch_upsample(const UpsampleArgs &u, bool lds, hipStream_t stream);
// panoramas (rt_panorama.hip; rt_panorama_device).  One launch, one thread per output pixel of the w x h frame: `tables` are the 2 w + 2 h
// doubles of rt_panorama_tables, `faces` six frames of 3 F F doubles, face-major; `out` gets 3 w h means.
void launch_panorama(int32_t w, int32_t h, const double *tables, const double *faces, int32_t face_size, int32_t guard, double inv_spp, double *out,
                     hipStream_t stream);
// frame metrics (rt_metrics.hip; rt_frame_error_device, rt_frame_noise_device).  Each runs every level of the normative 256-tree over
// the n_pixels entries that level 0 makes from the frames; `partials` has room for METRICS_ENTRY_DOUBLES 8-byte words per block of every
// level, level 0's first (rt_metrics_workspace_bytes); the last level writes the eight (four) final values to out8 (out4).
constexpr int METRICS_ENTRY_DOUBLES = 6; // a block's record: up to five accumulators and the count (a uint64) in the last word
void launch_frame_error(int64_t n_pixels, const double *values, double inv_spp, const int32_t *spp_map, const double *ref, double inv_ref, double eps,
                        double peak, double *partials, double *out8, hipStream_t stream);
void launch_frame_noise(int64_t n_pixels, bool means, const double *first, const double *second, int32_t n, const int32_t *spp_map, double eps,
                        double *partials, double *out4, hipStream_t stream);
void launch_debug_box(int64_t n,const double *rays, const double *boxes, double tmin, double tmax, uint8_t *exact_hit, uint8_t *f32_hit);
void launch_debug_quad(int64_t n, const double *rays, const Quad *quads, const QFiltPair *filt, double tmin, double tmax, uint8_t *exact_hit, uint8_t *keep);
// the wide visit on n cases whose records are image rows 0 .. n - 1 (lds == 0: 256-byte records; else the seven tables, n * 32 bytes per plane table)
struct DebugWideArgs {
    int64_t n;
    const double *rays, *boxes, *tmin, *tmax; // boxes: [n][4][6] f64, for the exact test
    const uint8_t *todo;
    const float *extents;                     // per case, or null: `extent` for all
    float extent;
    const uint4 *image;
    float *enter, *leave;
    uint8_t *hit, *degenerate, *exact;
    int8_t *chosen;
};
void launch_debug_wide(const DebugWideArgs &a, int lds);
void launch_debug_eval(int32_t op, int64_t n, const double *a, const double *b, double *out);

} // namespace rtk
