/* rt_amd_debug.h — test and tuning hooks of librt_amd.  NOT part of the drop-in boundary (include/rt_amd.h): a host
 * renderer never needs these.  tests/, tools/ and bench.py's work counters use them.
 *
 * The two setters change PROCESS-WIDE defaults (under a mutex): they exist for A/B runs in tests and tools; product code
 * passes rt_scene_options to rt_scene_create_ex instead. */
#ifndef RT_AMD_DEBUG_H
#define RT_AMD_DEBUG_H

#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: evaluates one of the device-side scalar functions of the normative arithmetic over host arrays
 * (out[i] = f(a[i], b[i])), so that tests can compare the GPU's results with the oracle's bit for bit.
 * For the two RNG ops, a[i] and b[i] carry the BIT PATTERNS of the 64-bit stream key and of the draw number
 * (0-based, as in "draw n" of the RNG definition below). */
typedef enum rt_debug_op {
    RT_DEBUG_LOG = 1, RT_DEBUG_SIN = 2, RT_DEBUG_ACOS = 3, RT_DEBUG_ATAN2 = 4 /* atan2(a, b) */, RT_DEBUG_POW5 = 5,
    RT_DEBUG_SQRT = 6, RT_DEBUG_DIV = 7 /* a / b */, RT_DEBUG_MUL_ADD = 8 /* a * b + a, two roundings */,
    RT_DEBUG_RNG_RANDOM = 9, RT_DEBUG_RNG_RANGE = 10 /* gen_range(-1.0..1.0) */,
    RT_DEBUG_F32_ABOVE = 11, RT_DEBUG_F32_BELOW = 12 /* the ordered walk's outward f32 conversions of an interval end (as doubles) */,
    RT_DEBUG_RNG_UNNEXT = 13 /* random() number `b` of stream `a` after two draws too many were made and taken back (Rng::unnext) */,
    /* The rejection samplers' accept / reject decision (rt_reject.hpp), on candidates given as RAW 64-bit draws, bit-cast into `a`:
     * candidate c of the unit sphere is a[3c .. 3c+2], of the unit disk a[2c .. 2c+1]; n counts array elements, b is not read.
     * VERDICTS: out[Kc] = the f32 classifier's verdict (0 certain reject, 1 certain accept, 2 uncertain), out[Kc + 1] = the exact f64
     * predicate (1: accepted).  COORDS: out[Kc + k] = the f64 coordinate the kernel builds from draw k. */
    RT_DEBUG_REJECT_SPHERE_VERDICTS = 14, RT_DEBUG_REJECT_SPHERE_COORDS = 15,
    RT_DEBUG_REJECT_DISK_VERDICTS = 16, RT_DEBUG_REJECT_DISK_COORDS = 17
} rt_debug_op;
int rt_debug_eval(int32_t op, int64_t n, const double *a, const double *b, double *out, int device);

/* Test hook: runs the kernel's conservative f32 box test and the exact f64 slab test on n (ray, box) pairs —
 * rays[i] = (origin xyz, direction xyz), boxes[i] = (lo xyz, hi xyz), interval (tmin, tmax) — and reports, per pair,
 * whether each test enters the box: out_f32_hit bit 0 = the reference-order walk's test, bits 1 and 2 = the ordered walk's
 * pair test with the box in slot 0 / slot 1.  The f32 tests must enter wherever the exact one does (tests/test_gpu_parity.py). */
int rt_debug_box_tests(int64_t n, const double *rays, const double *boxes, double tmin, double tmax,
                       uint8_t *out_exact_hit, uint8_t *out_f32_hit, int device);

/* Test hook: the quad stage's conservative f32 filter (rt_device_scene.h quad_pair_keep) and the exact f64 Quad::hit
 * (src/quad.rs:96-127) on n (ray, quad) pairs — rays[i] = (origin xyz, direction xyz), quads[i] = (Q xyz, u xyz, v xyz), the
 * derived fields as Quad::new computes them (src/quad.rs:24-27), interval [tmin, tmax].  out_exact_hit[i] = 1: the exact test
 * accepts; out_keep[i] bit 0 / bit 1: the filter keeps the quad in the first / second slot of its pair record; bit 2 / bit 3: it
 * claims alpha and beta certainly inside [0, 1] (the exact test then skips them); bit 4: the exact alpha and beta ARE inside (1 also
 * where the exact test ends before it gets to them).  The filter must keep whatever the exact test accepts, and may claim "inside"
 * only where bit 4 is set (tests/test_gpu_parity.py). */
int rt_debug_quad_filter_tests(int64_t n, const double *rays, const double *quads, double tmin, double tmax, uint8_t *out_exact_hit,
                               uint8_t *out_keep, int device);

/* Test hook (no GPU needed): runs the scene compiler and returns the records the device would walk — the f64 box each
 * carries after refitting (refit != 0) or as the reference has it (refit == 0), the outward-rounded f32 box actually
 * tested, the threaded links, and the bound of the record's own primitives — so that tests can check the compiler's
 * invariants (links, containment) on the CPU.  out_nodes may be NULL to query the count. */
typedef struct rt_debug_node {
    double lo[3], hi[3];           /* box of the record (f64) */
    float lo32[3], hi32[3];        /* what the kernel tests */
    double prim_lo[3], prim_hi[3]; /* bound of the leaf's own primitives (+inf/-inf if none) */
    uint32_t skip, kind, no_bbox, a, b, _pad;
} rt_debug_node;
int rt_debug_compiled_nodes(const rt_scene_desc *desc, int32_t refit, rt_debug_node *out_nodes, int64_t capacity,
                            int64_t *out_count);

/* Test / tuning hook: how scenes created from now on are walked.  ordered = 2: the library's own trees, nearest child
 * first — with media, a sequence of trees and media in the reference's scan order (DESIGN.md "Ordered layout"; a medium
 * inside a Translate / RotateY frame keeps the other walk); 0: every scene walks the reference's tree in the reference's
 * order; 1 (default): as 2, except for scenes measured faster the other way (a single primitive).
 * leaf_max > 0: primitives per leaf of those trees at most; 0: back to the default.  Negative: keep.
 * Affects speed only, never results. */
int rt_debug_set_traversal(int32_t ordered, int32_t leaf_max);

/* Test / tuning hook: which shortcuts the ordered walk of scenes created / rendered from now on takes (negative: keep).
 * flat_max: a frame of at most this many primitives keeps them in one leaf under its root (0: off; default 8) — scene creation;
 * start_shortcut: a query starts with the primitives of a leaf under the root that spans the scene (0 / 1) — per render;
 * defer_instances: the world frame's instances are walked after its own tree (0 / 1) — per render;
 * seq_lookahead: a query looks ahead at the later steps of the world's sequence when it starts (0 / 1) — per render;
 * slow_min, slow_age: hits on a noise texture wait in the shade stage for slow_min of their kind, at most slow_age shade rounds
 * (slow_min 1: nobody waits; defaults 4, 32) — per render.
 * Affects speed only, never results. */
int rt_debug_set_walk_shortcuts(int32_t flat_max, int32_t start_shortcut, int32_t defer_instances, int32_t seq_lookahead,
                                int32_t slow_min, int32_t slow_age);

/* Test / tuning hook: where the start shortcut's leaf is a single sphere, renders from now on run that sphere's test where a query
 * starts (1, the default; RT_START_INLINE) or in a round of the sphere stage (0); negative: keep.  Affects speed only, never results. */
int rt_debug_set_start_inline(int32_t start_inline);

/* Test hook: the ordered layout the scene compiler builds for `desc` (no device needed).  Set the cap_* fields and
 * the pointers (any may be null: only the counts are returned then).
 * nodes: 16 words per record = two boxes as 6 floats (x.lo, x.hi, y.lo, y.hi, z.lo, z.hi), two child references
 * (kind << 29 | (count - 1) << 26 | index; kind 0 record, 1 spheres, 2 quads, 3 instance, 7 empty), 2 unused.
 * spheres: 9 doubles = center, radius, center_vec, seq, is_moving.  quads: 10 = q, u, v, seq.
 * instances: 8 = offset, sin, cos, parent, flags (1 translate, 2 rotate), root record.
 * steps: the world frame's sequence, 28 words per step = kind (0 tree, 1 medium bounded by one sphere, 2 medium with a
 * boundary tree), a (tree: root record; medium: its index), b (boundary tree's root), moving, box as 6 floats, 2 unused,
 * then as doubles: the boundary sphere's center (3), radius, center_vec (3), and the medium's neg_inv_density.
 * media: per medium, the index of its boundary sphere (kind 1 steps). `root` is the first step's tree. */
typedef struct rt_debug_ordered {
    int64_t cap_nodes, cap_spheres, cap_quads, cap_instances, cap_steps, cap_media;
    int64_t n_nodes, n_spheres, n_quads, n_instances, n_steps, n_media;
    uint32_t ordered, root, stack_entries, _pad;
    uint32_t *nodes;
    double *spheres, *quads, *instances;
    uint32_t *steps, *media;
} rt_debug_ordered;
int rt_debug_ordered_layout(const rt_scene_desc *desc, rt_debug_ordered *io);
/* ... with the tree options of `options` (leaf_max, flat_max; NULL: the process defaults) */
int rt_debug_ordered_layout_ex(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_ordered *io);

/* Structure check of the four-child layout (rt_scene_options.wide), on the CPU: out[0] records, out[1] primitives found in leaves,
 * out[2] primitives in the scene's tables (a medium's boundary sphere solved in place is in no leaf), out[3] stack entries a walk needs,
 * out[4] violations (a primitive in no leaf or in two, a child record's boxes outside its slot's box, a bad reference, an empty slot
 * whose box a ray could enter), out[5] records on the longest chain. */
int rt_debug_wide_layout(const rt_scene_desc *desc, const rt_scene_options *options, uint64_t out[6]);

/* Test hook (no GPU needed): the four-child records a scene created from `desc` with `options` walks, as the device sees them.
 * Set cap_records / cap_steps and the pointers (any may be null: only the counts and scalars are returned then).  wide = 0: the
 * scene gets no four-child records under these options (n_records = 0).
 * boxes: per record and slot the f32 box (x.lo, x.hi, y.lo, y.hi, z.lo, z.hi); refs: the four references (rt_debug_ordered's
 * encoding; an empty slot: kind 7 and the box lo = +inf, hi = -inf).  bounds: in the same order, the f64 bound of what the slot
 * holds — a leaf's primitives, everything below an inner record, an instance's content seen from the enclosing frame; an empty
 * slot: (+inf, -inf).  box_extent: the B of the f32 box filter (every |plane| tested must be <= B), as scene creation computes it.
 * step_boxes: the boxes of the world frame's sequence, which the same filter tests.
 * global_image (256 bytes per record) and lds_image (table_bytes = 32 * n_records for each of the six plane tables X+ | X- | Y+ | Y-
 * | Z+ | Z-, each row the four planes a ray of that sign enters the children through, then the four it leaves through; then 16
 * bytes per record of references) are the two packed forms exactly as scene creation uploads them (the same function packs). */
typedef struct rt_debug_wide {
    int64_t cap_records, cap_steps;
    int64_t n_records, n_steps;
    uint32_t wide, table_bytes;
    float box_extent;
    uint32_t _pad;
    float *boxes;          /* [n_records][4][6] */
    uint32_t *refs;        /* [n_records][4] */
    double *bounds;        /* [n_records][4][6] */
    uint8_t *global_image; /* [n_records][256] */
    uint8_t *lds_image;    /* [n_records * 208] */
    float *step_boxes;     /* [n_steps][6] */
} rt_debug_wide;
int rt_debug_wide_records(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_wide *io);

/* Test hook (no GPU needed): the plan of the scene rt_scene_create_ex would make of `desc` under `options` — everything scene creation
 * decides and every byte it uploads (csrc/rt_scene_plan.hpp; the same options check, the same planner).
 * In: oimage, lds_image, aux_image, mats, insts with their capacities in bytes (any may be null: only sizes and digests are returned).
 * Out: the layout's scalars under the names rt_scene's launches read them by (o_root 0xfffffffe: no own tree to start in;
 * o_start_direct 0xffffffff: none; lds_off_qfilt 0: no filter records); the scene's stats as rt_scene_get_stats returns them;
 * level[0] / level[1]: a launch at LDS level 0 and at the scene's lds_level (what rt_scene_options.use_lds chooses between) — the
 * kernel's feature mask, its workgroup threads, whether the small tables (AUX) and the parked world rays go into the LDS, where the
 * regions of the dynamic LDS start (stacks, sequence, AUX, world rays, profile rows) and its size, plain and for the instrumented
 * kernel; images[0..3]: byte count and 64-bit FNV-1a digest of the node tables' global form, the LDS image, the AUX image and the
 * material table; tables[0..10]: the same for the tables uploaded as they are — nodes, sequence, spheres, quads, instances, media,
 * textures, Perlin tables, image records, texels, sRGB table. */
typedef struct rt_debug_plan_level {
    uint32_t lds_level, features, threads, aux_in_lds, world_in_lds;
    uint32_t stack_off, seq_off, aux_off, world_off, prof_off;
    uint32_t dynamic_lds_bytes, dynamic_lds_bytes_counted;
} rt_debug_plan_level;
typedef struct rt_debug_plan_bytes {
    uint64_t bytes, digest;
} rt_debug_plan_bytes;
typedef struct rt_debug_plan {
    int64_t cap_oimage, cap_lds_image, cap_aux_image, cap_mats, cap_insts;
    uint8_t *oimage, *lds_image, *aux_image, *mats, *insts;
    uint32_t features, parks_colours, has_instances, ordered, wide, o_root, n_oseq, o_stack, n_nodes;
    uint32_t o_start_stage, o_start_prim, o_start_end, o_start_rest, o_start_slot, o_start_direct;
    float box_extent;
    uint32_t lds_level, lds_off_node_b, lds_off_spheres, lds_off_quads, lds_off_qfilt, lds_prefix_bytes[4];
    uint32_t aux_bytes, aux_off[5];
    rt_scene_stats stats;
    rt_debug_plan_level level[2];
    rt_debug_plan_bytes images[4];
    rt_debug_plan_bytes tables[11];
} rt_debug_plan;
int rt_debug_scene_plan(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_plan *io);

/* Test hook: the visit of a four-child record as the render kernels make it (rt_device_scene.h: make_ray_pair32, load_oquad,
 * box_quad_f32 on the interval converted outward, wide_verdict with the ray's degenerate flag, wide_nearest), on n cases.
 * Per case: rays = (origin xyz, direction xyz), the interval (tmin[i], tmax[i]), todo[i] = the mask of the slots to look at.
 * The records come in one of two ways.
 *   boxes != NULL: four f64 boxes per case (x.lo, x.hi, y.lo, y.hi, z.lo, z.hi; lo > hi on any axis: an empty slot) and, if
 *   refs != NULL, their four references (an empty slot always gets the empty one; refs == NULL: a sphere leaf).  The boxes are
 *   rounded outward as the scene compiler rounds them and packed by the function scene creation packs with.
 *   boxes == NULL: records already packed, as rt_debug_wide_records returns them (global_image, lds_image, n_records), and
 *   record[i] = the record case i visits.
 * extent: the filter's B; 0: per case, the largest |coordinate| of the case's own f32 boxes.  lds = 0: load_oquad reads the
 * 256-byte records from global memory; otherwise the plane and reference tables, staged into the LDS a batch of records at a time.
 * Out, per case: enter / leave = box_quad_f32's distances; hit = the mask of the slots entered; chosen = the slot the walk goes
 * on with (-1: none); degenerate = the ray's flag; exact = per slot, whether the exact f64 slab test (box_miss_f64) enters the f64
 * box (packed records: the f32 planes widened).  tests/test_gpu_wide_visit.py holds these against a numpy reference. */
typedef struct rt_debug_wide_cases {
    int64_t n;
    const double *rays;          /* [n][6] */
    const double *tmin, *tmax;   /* [n] */
    const uint8_t *todo;         /* [n] */
    const double *boxes;         /* [n][4][6] or NULL */
    const uint32_t *refs;        /* [n][4] or NULL */
    const uint8_t *global_image, *lds_image; /* packed records (boxes == NULL) */
    int64_t n_records;
    const uint32_t *record;      /* [n] */
    float extent;
    int32_t lds;
    float *enter, *leave;        /* [n][4] */
    uint8_t *hit;                /* [n] */
    int8_t *chosen;              /* [n] */
    uint8_t *degenerate;         /* [n] */
    uint8_t *exact;              /* [n] */
} rt_debug_wide_cases;
int rt_debug_wide_visits(const rt_debug_wide_cases *io, int device);

/* How the calling thread's last render was launched: out[0] = the render-kernel launches it took (more than one when the sample
 * range did not fit the sample buffer; of an adaptive render: its last batch's), out[1] = LDS level, out[2] = workgroup threads,
 * out[3] = workgroups. */
int rt_debug_last_launch(uint32_t out[4]);

/* Which render kernel the calling thread's last render ran (filled where rt_debug_last_launch's figures are, so a refused call
 * leaves the earlier render's): out[0] = the kernel's feature mask (1 spheres, 2 quads, 4 frames, 8 media, 16 textures; 31: the
 * every-feature kernel), out[1] = LDS level (3: the scene whole, 1: the records, 0: nothing), out[2] = 1: the library's own trees,
 * 0: the reference's order, out[3] = 1: four-child records, out[4] = 1: the small tables in the LDS (AUX), out[5] = job mode
 * (0 dense, 1 pixel list, 2 views), out[6] = ids_ok (0: every attenuation is parked as a colour), out[7] = workgroup threads. */
int rt_debug_last_kernel(uint32_t out[8]);

/* How the queries of the calling thread's last render started (filled where rt_debug_last_kernel's figures are): out[0] = the start
 * shortcut's stage (1 spheres, 2 quads; 0: none, a query starts at the root), out[1], out[2] = the start leaf's primitives
 * [first, end), out[3] = 1: the launch asked for the inline start test (one sphere in the leaf, start_inline on).  The test runs
 * inline only where the kernel has it compiled: feature mask 1 with the library's own trees (out[0], out[2] of rt_debug_last_kernel);
 * every other kernel ignores the word and tests the leaf in its stage. */
int rt_debug_last_start(uint32_t out[4]);

/* Test hook: one convergence step of adaptive sampling (rt_render_adaptive) on chosen inputs — the three kernels and the scratch
 * layout of the render's own step, nothing rendered.  Host arrays in and out.  list: n_list entries (a positive multiple of 64),
 * pixel indices below n_pixels (< 2^27) or padding (anything else, by convention 0xffffffff); sum, sum_sq: 3 * n_pixels doubles;
 * n: the samples they hold; last != 0: the last schedule point (every listed pixel leaves).  spp (n_pixels, in/out): a listed pixel
 * that leaves gets n, nothing else is written.  list_out (n_list, in/out: uploaded first, so that entries the step leaves alone
 * show): the survivors in list order, then padding up to a multiple of 64.  *out_count: the survivors.
 * tests/test_gpu_adaptive_step.py holds these against a numpy reference. */
int rt_debug_adaptive_step(int64_t n_list, const uint32_t *list, int64_t n_pixels, const double *sum, const double *sum_sq, int32_t n,
                           int32_t last, double rel_threshold, double abs_threshold, int32_t *spp, uint32_t *list_out, uint32_t *out_count,
                           int device);

/* Profiling hook: where the last rt_render_device_counted call's waves spent their time.  For each scheduler stage
 * (box, sphere, quad, other, shade, new-job): rounds run, lanes active summed over those rounds, shader cycles (s_memtime)
 * summed over waves; then six parts of the shade / path-end rounds, cycles only (hit rebuild, unit-sphere rejection sampling,
 * texture, material + next ray, attenuation products + sample store, job hand-out + camera ray — the stage slots keep the
 * remainder: scheduling and the start of the next query). */
int rt_debug_stage_profile(uint64_t out[36]);

/* Profiling hook: the last rt_render_device_counted call's visits of four-child records (rt_scene_options.wide; all 0 for other
 * walks).  out[0]: first visits of a record.  out[1 + 3 * (b - 1) + o]: revisits of a record that was set aside with b of its
 * children still to look at (b = 1, 2, 3), by what the walk went on with: o = 0 an inner record, 1 a leaf or an instance, 2 nothing
 * (every child culled against the interval as it had shrunk).  out[10]: entries set aside as a record with the mask of its children
 * left; out[11]: entries set aside as the one inner child left itself (RT_WIDE_SETASIDE=1). */
int rt_debug_visit_stats(uint64_t out[12]);

/* Tuning hook: the wave scheduler's knobs (DESIGN.md "Scheduler").  A deferred stage runs once th/64 of a wave's
 * live lanes wait for it (th_new: the path-end / next-job stage); the box loop keeps running while th_box/64 of them are in
 * it; use_lds = 0 forces the
 * scene to be gathered from global memory even when it fits the LDS.  A negative threshold restores the built-in
 * per-scene-class preset; a negative use_lds keeps the current setting.
 * Affects speed only, never results.  Process-wide; not for concurrent use with renders. */
int rt_debug_set_tuning(int32_t th_prim, int32_t th_other, int32_t th_shade, int32_t th_box, int32_t use_lds,
                        int32_t th_new);

/* Test / tuning hook: the largest stride at which rt_bloom_device calls from now on run a level as ONE launch (the H pass of a tile and
 * its halo rows into the LDS, a barrier, the V pass from there) instead of two global passes: 0 (never), 1 or 2, whatever the frame;
 * negative: back to the built-in rule (strides 1 and 2 on frames of at least 512 tiles of 64 x 16 pixels, never on smaller ones).
 * Returns the value in force before the call (-1: the built-in rule); a max_stride above 2 counts as 2.
 * Affects speed only, never results.  Process-wide. */
int rt_debug_set_bloom_fused(int32_t max_stride);

/* Test / tuning hook: the kernel form of rt_robust_device calls from now on — the number of register slots its sorting network has: 4,
 * 8, 16 or 32 (any other positive value counts as the next of these above it, 32 at the most); a form with fewer slots than a call has
 * blocks cannot run it, and that call takes the smallest form that fits.  0 or negative: back to the built-in rule (the smallest form
 * that fits).  Returns the value in force before the call (0: the built-in rule).  Affects speed only, never results.  Process-wide. */
int rt_debug_set_robust_form(int32_t slots);

/* Test / tuning hook: the form of the upsample kernel that rt_upsample_device calls from now on launch, whatever the frame: 0 the direct
 * form (every tap read from the workspace's regions in global memory), 1 (or more) the LDS form (a tile's low records staged once);
 * negative: back to the built-in rule (the LDS form, which was the faster one at every size and guide set measured).
 * Returns the value in force before the call (-1: the built-in rule).  Affects speed only, never results.  Process-wide. */
int rt_debug_set_upsample_form(int32_t form);


#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_DEBUG_H */
