/*
 * rt_amd.h — C ABI of the MI355X path-tracing renderer (librt_amd.so).
 *
 * This is the drop-in boundary for the reference's per-pixel render loop.  The reference
 * (Husenap/rust-tracing) has no FFI; its seam is
 *
 *     pub fn render(camera: Arc<Camera>, world: Arc<dyn Hittable>, output_file_name: String)
 *                                                              (src/renderer.rs:12, called at src/main.rs:665)
 *
 * and, beneath it, the trait objects dyn Hittable (src/hittable.rs:45-48), dyn Material
 * (src/material.rs:11-16) and dyn Texture (src/texture.rs:12-14).  Trait objects cannot cross to a GPU,
 * so the boundary carries the same object graph as plain-old-data: every Rust struct that implements one
 * of the three traits becomes one POD record below (same fields, same meaning), and every
 * Arc<dyn Hittable/Material/Texture> becomes an index.  A Rust host produces these records by walking its
 * own objects (one `describe()` method per trait); nothing here is device-specific.
 * How the library lays the scene out in HBM/LDS is private to the library.
 *
 * Everything the renderer computes is f64 (reference: `pub type FP = f64`, src/common.rs:1).
 *
 * Conventions
 *   - all functions return 0 on success and a negative rt_status on failure; they never abort or unwind;
 *     rt_last_error() returns a thread-local message for the last failure on the calling thread.
 *   - every pointer passed in is borrowed for the duration of the call only; the library copies.
 *   - rt_scene handles are immutable after creation and may be rendered from concurrently; two
 *     concurrent renders must not share an output buffer.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2 /* 2: per-path RomuDuoJr streams (the normative RNG changed: frames differ from abi 1), scene options, gather */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1, /* null pointer, bad index, unsupported graph shape */
    RT_ERR_NO_DEVICE = -2,        /* no HIP device / device index out of range          */
    RT_ERR_HIP = -3,              /* a HIP runtime call failed (message has the HIP error string) */
    RT_ERR_OUT_OF_MEMORY = -4,
    RT_ERR_UNSUPPORTED = -5,      /* graph is valid but outside what the device path handles */
    RT_ERR_COMM = -6              /* RCCL is not available or one of its calls failed (message has its error string) */
} rt_status;

/* Vec3 / Point3 / Color (src/vec3.rs:8-16). */
typedef struct rt_vec3 { double x, y, z; } rt_vec3;

/* AABB = three Intervals (src/aabb.rs:9-14, src/interval.rs:5-9). */
typedef struct rt_aabb { double lo[3]; double hi[3]; } rt_aabb;

/* ---- Hittable graph -------------------------------------------------------------------------------
 * rt_ref stands in for Arc<dyn Hittable>: (kind, index into the array of that kind). */
typedef enum rt_hittable_kind {
    RT_HITTABLE_NONE = 0,
    RT_HITTABLE_SPHERE = 1,          /* src/sphere.rs:13-20            */
    RT_HITTABLE_QUAD = 2,            /* src/quad.rs:11-20              */
    RT_HITTABLE_LIST = 3,            /* HittableList, src/hittable.rs:50-54 */
    RT_HITTABLE_TRANSLATE = 4,       /* src/hittable.rs:81-85          */
    RT_HITTABLE_ROTATE_Y = 5,        /* src/hittable.rs:113-118        */
    RT_HITTABLE_BVH = 6,             /* BVHNode, src/bvh.rs:12-14      */
    RT_HITTABLE_CONSTANT_MEDIUM = 7  /* src/constant_medium.rs:14-18   */
} rt_hittable_kind;

typedef struct rt_ref { int32_t kind; int32_t index; } rt_ref;

/* Sphere (src/sphere.rs:13-20).  `center_vec`/`is_moving` as set by with_target (src/sphere.rs:34-46).
 * The bounding box lives in the BVH leaf that holds the sphere (src/bvh.rs:44), not here. */
typedef struct rt_sphere {
    rt_vec3 center;
    double radius;
    rt_vec3 center_vec;
    int32_t is_moving;
    int32_t material;
} rt_sphere;

/* Quad (src/quad.rs:11-20) with the derived fields exactly as Quad::new computes them
 * (src/quad.rs:24-27): normal = normalize(u x v), d = normal . q, w = n / (n . n). */
typedef struct rt_quad {
    rt_vec3 q, u, v, w, normal;
    double d;
    int32_t material;
    int32_t _pad;
} rt_quad;

/* HittableList (src/hittable.rs:50-54): objects = list_items[first .. first+count). */
typedef struct rt_list { int32_t first; int32_t count; } rt_list;

/* Translate (src/hittable.rs:81-85) and RotateY (src/hittable.rs:113-118; sin/cos of the angle as
 * RotateY::new stores them, src/hittable.rs:121-123). */
typedef struct rt_translate { rt_ref object; rt_vec3 offset; } rt_translate;
typedef struct rt_rotate_y { rt_ref object; double sin_theta; double cos_theta; } rt_rotate_y;

/* One `(Node, AABB)` pair of the BVH (src/bvh.rs:16-19).  is_leaf: Node::Leaf(object) else
 * Node::Branch(left, right) with left/right indexing bvh_nodes. */
typedef struct rt_bvh_node {
    rt_aabb bbox;
    int32_t is_leaf;
    int32_t left, right;
    rt_ref object;
    int32_t _pad;
} rt_bvh_node;

/* BVHNode (src/bvh.rs:12-14): root indexes bvh_nodes. */
typedef struct rt_bvh { int32_t root; int32_t _pad; } rt_bvh;

/* ConstantMedium (src/constant_medium.rs:14-18); phase_material indexes materials (an ISOTROPIC one). */
typedef struct rt_constant_medium {
    rt_ref boundary;
    double neg_inv_density;
    int32_t phase_material;
    int32_t _pad;
} rt_constant_medium;

/* ---- Materials (src/material.rs) ------------------------------------------------------------------ */
typedef enum rt_material_kind {
    RT_MATERIAL_LAMBERTIAN = 1,    /* :18-42   texture = albedo                 */
    RT_MATERIAL_METAL = 2,         /* :44-64   albedo, fuzz (not clamped)        */
    RT_MATERIAL_DIELECTRIC = 3,    /* :66-104  ir                                */
    RT_MATERIAL_DIFFUSE_LIGHT = 4, /* :106-122 texture = emit                    */
    RT_MATERIAL_ISOTROPIC = 5      /* :124-138 texture = albedo                  */
} rt_material_kind;

typedef struct rt_material {
    int32_t kind;
    int32_t texture; /* index into textures, or -1 */
    rt_vec3 albedo;  /* Metal */
    double fuzz;     /* Metal */
    double ir;       /* Dielectric */
} rt_material;

/* ---- Textures (src/texture.rs) -------------------------------------------------------------------- */
typedef enum rt_texture_kind {
    RT_TEXTURE_SOLID = 1,   /* :17-37   color                                   */
    RT_TEXTURE_CHECKER = 2, /* :39-70   inv_scale, even, odd (texture indices)  */
    RT_TEXTURE_IMAGE = 3,   /* :72-93   image index                             */
    RT_TEXTURE_NOISE = 4    /* :95-111  perlin index, scale                     */
} rt_texture_kind;

typedef struct rt_texture {
    int32_t kind;
    int32_t even, odd; /* Checker */
    int32_t image;     /* Image   */
    int32_t perlin;    /* Noise   */
    int32_t _pad;
    rt_vec3 color;     /* Solid   */
    double inv_scale;  /* Checker: 1/scale as CheckerTexture::new stores it (src/texture.rs:46) */
    double scale;      /* Noise   */
} rt_texture;

/* Perlin tables (src/perlin.rs:7-13): 256 un-normalised gradient vectors and three permutations. */
#define RT_PERLIN_POINTS 256
typedef struct rt_perlin {
    rt_vec3 ranvec[RT_PERLIN_POINTS];
    int32_t perm_x[RT_PERLIN_POINTS];
    int32_t perm_y[RT_PERLIN_POINTS];
    int32_t perm_z[RT_PERLIN_POINTS];
} rt_perlin;

/* Decoded image of an ImageTexture (src/texture.rs:72-81): RGB8, row-major, row 0 at the top, as
 * image::DynamicImage::get_pixel(i, j) addresses it (src/texture.rs:89). */
typedef struct rt_image {
    int32_t width, height;
    const uint8_t *rgb;
} rt_image;

/* ---- Scene ---------------------------------------------------------------------------------------- */
typedef struct rt_scene_desc {
    uint32_t abi_version; /* RT_ABI_VERSION */
    uint32_t _pad;
    rt_ref world;         /* what main hands to render(): the top-level BVHNode (src/main.rs:659-665) */

    int32_t n_spheres, n_quads, n_lists, n_list_items, n_translates, n_rotates, n_bvh_nodes, n_bvhs,
        n_media, n_materials, n_textures, n_perlins, n_images;
    int32_t _pad2;

    const rt_sphere *spheres;
    const rt_quad *quads;
    const rt_list *lists;
    const rt_ref *list_items;
    const rt_translate *translates;
    const rt_rotate_y *rotates;
    const rt_bvh_node *bvh_nodes;
    const rt_bvh *bvhs;
    const rt_constant_medium *media;
    const rt_material *materials;
    const rt_texture *textures;
    const rt_perlin *perlins;
    const rt_image *images;
} rt_scene_desc;

/* Camera: the twelve fields of `pub struct Camera` after Camera::new (src/camera.rs:38-51, :54-110). */
typedef struct rt_camera {
    int32_t image_width, image_height;
    int32_t samples_per_pixel, max_depth;
    rt_vec3 background;
    rt_vec3 center;
    rt_vec3 pixel00_loc;
    rt_vec3 pixel_delta_u, pixel_delta_v;
    double defocus_angle;
    rt_vec3 defocus_disk_u, defocus_disk_v;
} rt_camera;

/* Output layouts. */
typedef enum rt_out_layout {
    /* out[(j*w + i)*3 + c]: exactly the reference's Vec<Color> (src/renderer.rs:32-33,:49).  Only the
     * pixels of this shard's tiles are written (all pixels when shard_count == 1). */
    RT_OUT_FRAME = 0,
    /* out[((lt*tile_h + ty)*tile_w + tx)*3 + c], lt = local tile number: tile k of the frame
     * (k = tile_row*tiles_per_row + tile_col) belongs to shard k % shard_count and is that shard's local
     * tile k / shard_count.  Edge tiles are padded to tile_w x tile_h; padding is written as 0.
     * This is the buffer each GPU contributes to the frame-end gather. */
    RT_OUT_TILES = 1
} rt_out_layout;

#define RT_TILE_W 8
#define RT_TILE_H 8

typedef struct rt_render_params {
    uint64_t seed;        /* render seed: keys the per-(pixel, sample) random stream (see RNG below) */
    int32_t sample_begin; /* samples [sample_begin, sample_end) of every pixel are traced and summed in order */
    int32_t sample_end;   /* <= 0: camera.samples_per_pixel */
    int32_t max_depth;    /* <= 0: camera.max_depth */
    int32_t accumulate;   /* 0: out = sum over the range; 1: out += (continues a previous range bit-exactly:
                             the per-pixel sum is a sequential f64 += over samples, src/renderer.rs:35-40) */
    int32_t shard_index;  /* this caller renders the tiles k with k % shard_count == shard_index */
    int32_t shard_count;  /* <= 0: 1 */
    int32_t out_layout;   /* rt_out_layout */
    int32_t device;       /* HIP device ordinal for rt_render (host-buffer form); ignored by rt_render_device,
                             which runs on the scene's device */
} rt_render_params;

/* Work counters of one render call (instrumented kernel; summed over all traced samples). */
typedef struct rt_counters {
    uint64_t samples;       /* camera paths traced                                          */
    uint64_t rays;          /* closest-hit queries issued by ray_color (src/renderer.rs:144) */
    uint64_t node_visits;   /* bounding-box tests; ordered walk: records visited (two boxes each) */
    uint64_t sphere_tests;
    uint64_t quad_tests;
    uint64_t medium_visits; /* ConstantMedium::hit entries (src/constant_medium.rs:34)       */
    uint64_t rng_draws;
    uint64_t noise_evals;   /* NoiseTexture::value calls                                     */
    uint64_t image_lookups; /* ImageTexture::value calls                                     */
    uint64_t instance_enters;
} rt_counters;

typedef struct rt_scene rt_scene; /* opaque; owned by the library */

/* Number of HIP devices visible to the library (0 if none; never an error). */
int rt_device_count(void);

/* Validates `desc`, compiles it into the device layout and uploads it to HIP device `device`.
 * Replaces: the Arc<dyn Hittable> world + Arc<Camera> hand-off at src/main.rs:659-665. */
int rt_scene_create(const rt_scene_desc *desc, int device, rt_scene **out_scene);
void rt_scene_destroy(rt_scene *scene);

/* Per-scene options (all optional: rt_scene_options_init fills the defaults; results never depend on them, only speed and
 * memory use do).  They replace the process-wide setters that round 1 used for this. */
typedef enum rt_walk {
    RT_WALK_DEFAULT = -1,        /* the library's default (RT_WALK_AUTO unless RT_ORDERED is set in the environment) */
    RT_WALK_REFERENCE_ORDER = 0, /* the reference's tree in the reference's order (src/bvh.rs:97-108), stackless */
    RT_WALK_AUTO = 1,            /* the library's own trees where they measured faster (DESIGN.md "Ordered layout") */
    RT_WALK_OWN_TREES = 2        /* the library's own trees wherever the scene allows it */
} rt_walk;
typedef struct rt_scene_options {
    uint32_t struct_size;        /* sizeof(rt_scene_options) as the CALLER was compiled: lets the struct grow compatibly — the library
                                    reads that many bytes and takes its defaults for every field beyond them */
    int32_t walk;                /* rt_walk */
    int32_t leaf_max;            /* own trees: primitives per leaf at most (<= 0: default) */
    int32_t refit;               /* -1 default (on); 0: keep the reference's boxes; 1: shrink them to the geometry */
    int32_t use_lds;             /* -1 default (on); 0: gather the scene from global memory even if it fits the LDS */
    int32_t th_prim, th_other, th_shade, th_box, th_new; /* scheduler thresholds in 64ths of a wave's live lanes; -1: preset */
    int64_t sample_buffer_bytes; /* per-(scene, stream) sample buffer at most; <= 0: default (2 GiB).  A frame that needs
                                    more is rendered in several launches over sample sub-ranges (same result). */
    int32_t reserved_pool;       /* ignored (rounds 2-3: the opt-in pool kernel, measured at 0.55x and removed — DESIGN_HISTORY.md); keeps
                                    the offsets of the fields below */
    int32_t flat_max;            /* own trees: a frame of at most this many primitives of one kind keeps them in one leaf under its root
                                    (0: off; -1: default, 8) */
    /* how the walk of the library's own trees starts and ends its queries (each -1: default) */
    int32_t start_shortcut;      /* 1: a query starts with the primitives of a leaf under the root that spans the scene */
    int32_t defer_instances;     /* 1: the world frame's Translate / RotateY subtrees are walked after the world's own tree */
    int32_t seq_lookahead;       /* 1: scenes with media: a query that cannot reach a later step of the world's sequence ends it early */
    int32_t slow_min, slow_age;  /* hits on a noise texture wait in the shade stage for slow_min of their kind, at most slow_age shade
                                    rounds (slow_min 1: nobody waits) */
    int32_t wide;                /* own trees: 1: records of four children, 0: of two; -1: default — four for scenes of 64 primitives or
                                    more (DESIGN.md "Wide records") */
    int32_t quad_filter;         /* -1 default (on); 0: every quad of a multi-quad leaf gets the exact test at once, without the conservative
                                    f32 filter in front of it (DESIGN.md "Quad filter") */
    int32_t medium_first;        /* -1 default (on); 0: off.  Own trees, scenes with media: a ray that starts inside the ball of a sphere-bounded
                                    medium makes that medium's draw before the tree in front of it is walked, and walks the tree no further
                                    than the draw's candidate (same results) */
} rt_scene_options;
/* Fills the defaults.  rt_scene_options_init writes sizeof(rt_scene_options) of THIS header: caller and library must have been built
 * from the same header.  A caller that may meet a newer library calls rt_scene_options_init_sized(&o, sizeof o) instead: only
 * that many bytes are written, struct_size is set to it, and rt_scene_create_ex treats the fields beyond it as default. */
void rt_scene_options_init(rt_scene_options *options);
int rt_scene_options_init_sized(rt_scene_options *options, uint32_t struct_size);
int rt_scene_create_ex(const rt_scene_desc *desc, int device, const rt_scene_options *options /* NULL: defaults */,
                       rt_scene **out_scene);

/* Bytes of device memory the compiled scene occupies, by part (for DESIGN.md's layout table). */
typedef struct rt_scene_stats {
    uint64_t node_bytes, sphere_bytes, quad_bytes, instance_bytes, medium_bytes, material_bytes,
        texture_bytes, perlin_bytes, image_bytes;
    uint32_t n_nodes, n_spheres, n_quads, n_instances, n_media, max_instance_depth;
    uint32_t lds_nodes, lds_bytes;      /* records resident in the LDS; LDS bytes a workgroup uses (image + stacks) */
    uint32_t ordered, stack_entries;    /* 1: the scene is walked through the library's own trees (DESIGN.md "Ordered walk") */
} rt_scene_stats;
int rt_scene_get_stats(const rt_scene *scene, rt_scene_stats *out);

/* The render loop (replaces src/renderer.rs:26-49, ray_color :139-155 and everything they call).
 * `out_rgb_sum` is a HOST buffer of rt_out_size() doubles holding per-pixel SUMS over the sample range —
 * the caller divides by spp and applies color_to_rgb exactly as src/renderer.rs:55-58 does.
 * Blocking; includes the device->host copy. */
int rt_render(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
              double *out_rgb_sum);

/* Same, but `d_out_rgb_sum` is DEVICE memory on the scene's device and the work is enqueued on
 * `hip_stream` (a hipStream_t; NULL = the null stream) without synchronising. */
int rt_render_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                     double *d_out_rgb_sum, void *hip_stream);

/* As rt_render_device with the instrumented kernel; blocks until done and fills `out_counters`
 * (results in d_out_rgb_sum are identical to the un-instrumented kernel's). */
int rt_render_device_counted(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                             double *d_out_rgb_sum, void *hip_stream, rt_counters *out_counters);

/* Number of doubles an output buffer needs for (width, height, layout, shard_index, shard_count). */
int64_t rt_out_size(int32_t width, int32_t height, int32_t out_layout, int32_t shard_index,
                    int32_t shard_count);

/* Frame-end reassembly on the device: `d_gathered` holds shard 0's RT_OUT_TILES buffer, then shard 1's, ...
 * each padded to rt_out_size(w, h, RT_OUT_TILES, 0, shard_count) doubles (shard 0 has the most tiles);
 * writes the RT_OUT_FRAME image into d_frame.  Enqueued on hip_stream. */
int rt_tiles_to_frame_device(int32_t width, int32_t height, int32_t shard_count, const double *d_gathered,
                             double *d_frame, void *hip_stream);

/* Output stage on the device (reference: color_to_rgb(c / spp), src/renderer.rs:55-58, src/color.rs:12-19):
 * rgb8[k] = (u8)(256 * clamp(gamma(sum[k] * (1/spp)), 0, 0.999)) for each of the n_values channel sums, with gamma(x) =
 * x^(1/2.2) by the fixed algorithm of "Normative definitions" below — the same code the host library runs
 * (rth_resolve_rgb8), so device and host bytes are identical.  Elementwise: works on a frame (3 * w * h values) and on a
 * shard's RT_OUT_TILES buffer alike.  Enqueued on hip_stream. */
int rt_resolve_rgb8_device(int32_t width, int32_t height, int32_t spp, const double *d_frame_sum,
                           uint8_t *d_rgb8, void *hip_stream);
int rt_resolve_rgb8_values_device(int64_t n_values, int32_t spp, const double *d_sum, uint8_t *d_rgb8, void *hip_stream);
/* rt_tiles_to_frame_device for gathered RGB8 tile buffers (one byte per value instead of one double). */
int rt_tiles_to_frame_rgb8_device(int32_t width, int32_t height, int32_t shard_count, const uint8_t *d_gathered,
                                  uint8_t *d_frame, void *hip_stream);

/* ---- adaptive sampling (opt-in; nothing above changes) --------------------------------------------------------------
 * A path's random stream is keyed by (seed, pixel, sample) and a pixel's sum is a sequential += over its samples in order, so a
 * pixel that stops after n samples holds, bit for bit, the sum a uniform render at spp = n gives that pixel.
 *
 * rt_render_pixels_device renders the samples [sample_begin, sample_end) of the listed pixels only: for each entry p of d_pixels
 * (n_pixels entries, device memory; pixel = j * width + i) the samples are added in order onto d_sum[3 p ..] (a frame of
 * 3 * w * h doubles; continuing its value when params->accumulate is set) and, if d_sum_sq is not NULL, each sample's c * c (the
 * product rounded, then added) onto d_sum_sq[3 p ..] likewise.  Entries >= w * h (0xFFFFFFFF: padding) trace nothing; pixels not
 * in the list are never written.  A pixel listed twice is the caller's error (its sums are then undefined).  Needs w * h < 2^27,
 * shard_count 1 and out_layout RT_OUT_FRAME.  Enqueued on hip_stream.
 *
 * rt_render_adaptive renders every pixel from sample 0 up to max_spp = params->sample_end (camera->samples_per_pixel when that is
 * <= 0), but stops a pixel early once its estimate has converged.  The evaluation points are n_k = min(min_spp + k * batch_spp,
 * max_spp); at each, every still-active pixel that is converged, or has reached max_spp, gets spp = n_k and stops.  The rule, f64 in
 * this order without FMA, for n >= 2 samples with sums S_c and squared sums Q_c:
 *     m_c = S_c / n;  v_c = (Q_c - S_c * m_c) / (n - 1);  e2 = max(v_r, v_g, v_b) / n;  L = ((m_r + m_g) + m_b) / 3
 *     tol = rel_threshold * L + abs_threshold;  converged <=> e2 <= tol * tol     (a non-finite S or Q never converges)
 * Outputs: the frame's sums (each pixel's = the uniform render's at its own spp), the per-pixel spp (w * h int32), optionally the
 * sums of squares, and the totals.  Needs sample_begin 0, accumulate 0, shard_count 1; min_spp is clipped to max_spp and must be
 * >= 2 when max_spp >= 2.  Both forms block: the device form reads one 4-byte count of still-active pixels per batch (one
 * synchronisation of hip_stream per batch) and returns when the last batch is done.  Resolve with rt_resolve_rgb8_spp_device. */
typedef struct rt_adaptive_params {
    uint32_t struct_size;   /* sizeof(rt_adaptive_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t min_spp;        /* first evaluation point (default 16) */
    int32_t batch_spp;      /* samples between evaluation points (default 16) */
    int32_t _pad;
    double rel_threshold;   /* default 0.02 */
    double abs_threshold;   /* default 1e-3 */
} rt_adaptive_params;
typedef struct rt_adaptive_result {
    int64_t samples;        /* camera paths traced (= the sum of the spp map) */
    int32_t launches;       /* evaluation points reached (render launches) */
    int32_t converged;      /* pixels the rule stopped before max_spp */
} rt_adaptive_result;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_adaptive_params_init_sized(rt_adaptive_params *params, uint32_t struct_size);
int rt_render_pixels_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const uint32_t *d_pixels,
                            int32_t n_pixels, double *d_sum, double *d_sum_sq /* NULL: none */, void *hip_stream);
int rt_render_adaptive(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params, const rt_adaptive_params *adaptive,
                       double *out_rgb_sum, int32_t *out_spp, double *out_rgb_sum_sq /* NULL: none */, rt_adaptive_result *out_result);
int rt_render_adaptive_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                              const rt_adaptive_params *adaptive, double *d_sum, int32_t *d_spp, double *d_sum_sq /* NULL: none */,
                              void *hip_stream, rt_adaptive_result *out_result);
/* color_to_rgb(sum / spp[pixel]) over a frame: a pixel with spp n gets the bytes rt_resolve_rgb8_device gives at spp = n. */
int rt_resolve_rgb8_spp_device(int32_t width, int32_t height, const double *d_sum, const int32_t *d_spp, uint8_t *d_rgb8,
                               void *hip_stream);

/* ---- views: many cameras of one scene in a single launch (opt-in; nothing above changes) ----------------------------------------
 * A small frame does not fill the machine, and a caller who renders many of them — a turntable, a stereo pair, the faces of a cube map
 * — pays launch, ramp-up, tail and summation once per frame.  rt_render_views_device renders n_views cameras of one scene as ONE job
 * space (view v's tiles behind view v - 1's), so the machine stays full from the first view to the last.
 *
 * View v is, bit for bit, the frame rt_render gives under (views[v].camera, seed = views[v].seed): d_out[v * 3wh ..] equals what
 * rt_render_device(scene, &views[v].camera, params with seed = views[v].seed, ...) writes there.  params->seed is IGNORED; sample_begin,
 * sample_end, max_depth and accumulate mean what they mean for rt_render_device and apply to every view.  `views` is HOST memory and is
 * copied during the call.  RT_ERR_INVALID_ARGUMENT (the message names the field), before any device work: n_views < 1; a null pointer;
 * cameras that differ in image_width or image_height; cameras that differ in samples_per_pixel (max_depth) while params->sample_end
 * (params->max_depth) is <= 0; shard_count > 1; an out_layout other than RT_OUT_FRAME.  RT_ERR_UNSUPPORTED, likewise before any
 * allocation: n_views x tiles per frame >= RT_VIEWS_MAX_TILES — a job's row (tile x sample) must stay below 2^27 for the kernel's exact
 * reciprocal decode and the job count, 64 per row, below 2^31 (the job index has 32 bits; launches keep half of them as headroom for
 * the grabs past the end), at the one sample per launch that chunking can always fall back to —
 * and, as for any render, a batch of which not even one sample per pixel fits the sample buffer.
 * rt_render_views_device enqueues on hip_stream and does not synchronise; rt_render_views blocks and downloads (with accumulate set,
 * `out` is uploaded first). */
typedef struct rt_view {
    rt_camera camera;
    uint64_t seed;
} rt_view;   /* view v is, bit for bit, the frame rt_render gives under (camera, seed) */
#define RT_VIEWS_MAX_TILES (1 << 25) /* min(2^27 rows, 2^31 jobs / 64 per row) */
int rt_render_views_device(const rt_scene *scene, const rt_view *views /* HOST, n_views entries, copied */, int32_t n_views,
                           const rt_render_params *params, double *d_out /* n_views frames of 3*w*h doubles, view-major */, void *hip_stream);
int rt_render_views(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params,
                    double *out /* host */);

/* ---- live refinement: a running-mean frame and its RGBA8 display bytes (opt-in; nothing above changes) ----------------------------
 * The reference's second entry point, live_render (src/renderer.rs:77-137, the CLI's -l/--live), refines the frame it shows one sample
 * per displayed frame with a running mean,  avg += (new - avg) / num_samples  (:114), and shows color_to_rgb(avg) with alpha 0xff
 * (:124-126).  That is a different f64 recurrence from rt_render's sum / n: a subtraction, a correctly rounded division and an addition
 * per sample, each rounded on its own ("Arithmetic" below: no reciprocal multiply, no contraction).  The window stays with the host;
 * these calls give it, per pass, the updated mean and the bytes to blit.
 *
 * rt_render_mean_device traces the samples [sample_begin, sample_end) of every pixel — the streams rt_render traces, keyed by (seed,
 * pixel, sample) — and folds them into d_mean (a frame of 3 * w * h doubles, d_mean[(j*w + i)*3 + c]) in order:
 *     for s = sample_begin .. sample_end - 1:   m = m + (c_s - m) / (double)(s + 1)
 * sample_begin is therefore also the number of samples already in the mean: m starts from +0.0 when it is 0 (d_mean's previous
 * content is then not read) and from d_mean's value otherwise, so a call over [0, a) followed by one over [a, b) equals one over
 * [0, b) bit for bit.  (The division is the one written at :114, IEEE-rounded; the reference's own `Vec3 / FP` multiplies by 1.0 / rhs,
 * src/vec3.rs:244-249, which differs in the last bit of some values.)  sample_end <= 0 means camera->samples_per_pixel.  If d_rgba8 is not NULL (4 * w * h bytes, 4-byte aligned), the
 * display frame of the mean the call arrives at is written with it, in the same pass over the samples: bytes 4p + 0..2 of pixel p are
 * what rt_resolve_rgb8_device gives at spp = 1 for values 3p + 0..2, byte 4p + 3 is 0xff.  Enqueued on hip_stream, not synchronised;
 * split into launches, pipelined and sized as rt_render_device is.  rt_render_mean blocks and downloads; when sample_begin > 0 it
 * uploads `mean` first.  rt_resolve_rgba8_device is the display stage alone, for callers who keep their own mean.
 * RT_ERR_INVALID_ARGUMENT (the message names the field), before the scene handle or any device work is touched: a null pointer other
 * than d_rgba8 / rgba8; accumulate != 0 (the mode continues through sample_begin); shard_count > 1; an out_layout other than
 * RT_OUT_FRAME; sample_begin < 0 or an empty sample range; a d_rgba8 that is not 4-byte aligned. */
int rt_render_mean_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                          double *d_mean /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *hip_stream);
int rt_render_mean(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                   double *mean /* host; read when sample_begin > 0 */, uint8_t *rgba8 /* host, or NULL */);
int rt_resolve_rgba8_device(int32_t width, int32_t height, const double *d_mean, uint8_t *d_rgba8, void *hip_stream);

/* ---- denoise: per-pixel moments of a frame and a variance-guided à-trous filter (opt-in; nothing above changes) -----------------------
 * Adaptive sampling, views and live refinement all produce frames of few samples per pixel; these calls make such a frame showable.
 *
 * rt_render_moments_device renders the samples [sample_begin, sample_end) of every pixel and writes two frames of 3 * w * h doubles:
 * d_sum is, bit for bit, what rt_render_device writes; d_sum_sq holds per channel the in-order sum of each sample's c * c (the product
 * rounded, then added: rt_render_pixels_device's definition).  params->accumulate continues both.  It is list mode over the list of
 * every pixel in tile order, with list mode's limits: w * h < 2^27, shard_count 1, out_layout RT_OUT_FRAME — otherwise, and for a null
 * pointer, RT_ERR_INVALID_ARGUMENT (the message names the field) before the scene handle or any device work is touched.  Enqueued on
 * hip_stream; the scene keeps the pixel list of a frame size, so only the first call at a size allocates (and waits for the list once).
 * rt_render_moments blocks and downloads; with accumulate set it uploads both buffers first.
 *
 * rt_denoise_device needs no scene: it filters the frame of means S / n that (d_sum, d_sum_sq, sample counts) describe, guided by the
 * variance of each pixel's mean, and writes the filtered means (and optionally their display bytes).  It is enqueued on hip_stream, does
 * not synchronise and does not allocate: d_workspace is rt_denoise_workspace_bytes(w, h) bytes of device memory (16-byte aligned) that the
 * caller owns.  RT_ERR_INVALID_ARGUMENT (the field named) before any device work: width or height < 1 or w * h >= 2^27; a null d_sum,
 * d_sum_sq, d_mean_out or d_workspace; spp < 2 when d_spp is NULL; a struct_size this library does not know; iterations outside 1..6;
 * sigma or eps that is not a number > 0; d_mean_out overlapping d_sum or d_sum_sq; a d_rgba8 that is not 4-byte aligned.
 *
 * Normative definition.  All arithmetic is f64, every operation rounded on its own ("Arithmetic" below: no FMA, IEEE division and
 * square root), max(a, b) = (b > a ? b : a).  p is a pixel, n its sample count (spp, or d_spp[p]) as a double.
 *   Prepare.   m_c = S_c / n.  p is VALID iff n >= 2 and all six of S_c, Q_c are finite.  For a valid pixel
 *              v_c = (Q_c - S_c * m_c) / (n - 1)          (the adaptive rule's terms)
 *              V0 = max(max(max(v_r, v_g), v_b), 0) / n;   C0 = m.
 *              A pixel that is not valid keeps C = m through every iteration, is written to the output unchanged and is never a tap.
 *   Iteration k = 0 .. K - 1, stride s = 2^k, for every valid p, with L(x) = ((C_r + C_g) + C_b) / 3 of C_k:
 *              G  = [sum of (g[dy] * g[dx]) * V_k(q)] / [sum of g[dy] * g[dx]], g = (1/4, 1/2, 1/4), over the in-frame valid pixels
 *                   q = p + (dx, dy), dy = -1..1 outer, dx = -1..1 inner (offsets of one pixel at every stride); both sums start at 0
 *              sd = sqrt(G);  den = sigma * sd + eps
 *              sw = sc_c = sv = 0; then for dy = -2..2 outer, dx = -2..2 inner, q = p + s * (dx, dy), skipping q out of frame or not valid,
 *              with h = (1/16, 1/4, 3/8, 1/4, 1/16):
 *                   x = |L(p) - L(q)| / den;  t = 1 - x * x;  e = (t > 0 ? t * t : 0);  w = (h[dy] * h[dx]) * e
 *                   sw = sw + w;  sc_c = sc_c + w * C_k(q)_c;  sv = sv + (w * w) * V_k(q)
 *              C_k+1(p) = sc / sw;  V_k+1(p) = sv / (sw * sw)           (sw >= 9/64: the centre tap has e = 1)
 *   Output.    d_mean_out = C_K (3 * w * h doubles); d_rgba8, if not NULL, the bytes rt_resolve_rgba8_device gives for C_K, written by
 *              the last iteration itself. */
typedef struct rt_denoise_params {
    uint32_t struct_size;   /* sizeof(rt_denoise_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t iterations;     /* K, 1..6 (default 4): strides 1, 2, 4, ... 2^(K-1) */
    double sigma;           /* edge-stopping width in standard deviations of the mean (default 4.0), > 0 */
    double eps;             /* added to the denominator (default 1e-6), > 0 */
} rt_denoise_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_denoise_params_init_sized(rt_denoise_params *params, uint32_t struct_size);
/* Bytes of device memory rt_denoise_device needs for a w x h frame (two halves of 4 doubles per pixel); -1 for a size it refuses. */
int64_t rt_denoise_workspace_bytes(int32_t width, int32_t height);
int rt_denoise_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp,
                      const int32_t *d_spp /* NULL: uniform spp */, const rt_denoise_params *params /* NULL: defaults */,
                      double *d_mean_out /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int rt_render_moments_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                             double *d_sum /* 3*w*h */, double *d_sum_sq /* 3*w*h */, void *hip_stream);
int rt_render_moments(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                      double *sum /* host */, double *sum_sq /* host */);

/* ---- albedo scene and albedo-guided denoise (opt-in; nothing above changes) ------------------------------------------------------------
 * The filter above stops at edges of the noisy luminance only, so it cannot tell a texture from noise.  A first-hit ALBEDO frame can:
 * the frame is divided by it, the texture-free irradiance that is left is filtered (stopping at albedo edges as well), and the albedo
 * is multiplied back in.
 *
 * Albedo scene.  The albedo frame needs no new render path: it is an ordinary render of the ALBEDO SCENE of a description, the same
 * geometry with every material turned into a DIFFUSE_LIGHT that emits the original's albedo texture.  A light does not scatter, so
 * ray_color returns the first hit's albedo and the path ends there; the RNG is keyed by (seed, pixel, sample) and the camera's and the
 * media's draws come before a material's, so path (seed, p, s) of the albedo scene meets the first hit of path (seed, p, s) of the
 * original — defocus, motion blur and the random hit inside a constant medium included.  Normative rule (rt_albedo_materials):
 *   out_textures[0 .. n_textures) is a copy of desc->textures.  Then, for materials k = 0, 1, ... in order:
 *     LAMBERTIAN or ISOTROPIC with texture t  ->  {DIFFUSE_LIGHT, texture t}
 *     METAL                                   ->  {DIFFUSE_LIGHT, texture = a newly appended SOLID of colour `albedo`}
 *     DIELECTRIC                              ->  {DIFFUSE_LIGHT, texture = a newly appended SOLID of colour (1, 1, 1)}
 *     DIFFUSE_LIGHT                           ->  copied as it is
 *   Appended textures come in material order, one per metal or dielectric, behind the copies: {kind SOLID, even = odd = image =
 *   perlin = -1, _pad 0, color, inv_scale 0, scale 0}.  albedo, fuzz and ir of a rewritten material are zero.
 *   *out_n_textures = n_textures + (metals + dielectrics).
 * rt_albedo_materials touches no device.  RT_ERR_INVALID_ARGUMENT (the message names the field), as rt_scene_create gives it: a null
 * desc, out_materials, out_textures or out_n_textures; abi_version other than RT_ABI_VERSION; a negative n_materials or n_textures,
 * or a null materials / textures array with a non-zero count; a materials[k].kind that is none of the five; a materials[k].texture
 * out of range for a kind that reads one.  Nothing is written then.
 * rt_scene_create_albedo is rt_scene_create_ex on `desc` with those two arrays and n_textures swapped in: geometry, trees and options
 * are the caller's.  The kernel a scene is rendered by depends on its geometry and on whether any texture is not a SOLID, not on
 * material kinds, and the appended textures are SOLID: an albedo scene is rendered by the kernel of its original.
 * The caller's CAMERA decides what a miss contributes: the albedo frame of a pixel whose paths leave the scene is the camera's
 * background.  The layers above this ABI render the albedo scene with the beauty camera and background = (1, 1, 1), so that a
 * background pixel's divisor is 1 and it demodulates to the background colour itself. */
int rt_albedo_materials(const rt_scene_desc *desc, rt_material *out_materials /* desc->n_materials */,
                        rt_texture *out_textures /* room for desc->n_textures + desc->n_materials */, int32_t *out_n_textures);
int rt_scene_create_albedo(const rt_scene_desc *desc, int device, const rt_scene_options *options /* NULL: defaults */,
                           rt_scene **out_scene);

/* rt_denoise_albedo_device is rt_denoise_device with an albedo frame beside the moments: d_albedo_sum holds 3 * w * h doubles, the
 * per-pixel sums of albedo_spp samples of the albedo scene (what rt_render_device writes for it).  The contract is rt_denoise_device's:
 * enqueued on hip_stream, not synchronised, nothing allocated; d_workspace is rt_denoise_albedo_workspace_bytes(w, h) bytes of device
 * memory, 16-byte aligned.  RT_ERR_INVALID_ARGUMENT (the field named) before any device work: everything rt_denoise_device refuses,
 * and a null d_albedo_sum; albedo_spp < 1; a sigma_albedo or albedo_floor that is not a number > 0; d_mean_out overlapping
 * d_albedo_sum.
 *
 * Normative definition.  All arithmetic is f64, every operation rounded on its own (no FMA, IEEE division and square root),
 * max(a, b) = (b > a ? b : a).  p is a pixel, n its sample count (spp, or d_spp[p]) and n_a = albedo_spp, as doubles; S, Q, A are p's
 * entries of d_sum, d_sum_sq, d_albedo_sum.
 *   Prepare.   m_c = S_c / n;  a_c = A_c / n_a.  p is VALID iff n >= 2 and all nine of S_c, Q_c, A_c are finite.  For a valid pixel
 *              d_c = max(a_c, albedo_floor)                   (the divisor)
 *              I_c = m_c / d_c                                 (the irradiance)
 *              v_c = (Q_c - S_c * m_c) / (n - 1);   u_c = v_c / (d_c * d_c)
 *              V0 = max(max(max(u_r, u_g), u_b), 0) / n;   C0 = I.
 *              A pixel that is not valid keeps C = m through every iteration, is written to the output unchanged and is never a tap.
 *   Iteration k = 0 .. K - 1, stride s = 2^k: exactly the iteration of rt_denoise_device on (C_k, V_k) — G, sd, den, the 25 taps with dy
 *              outer and dx inner, x, t and e as defined there — with one more factor per tap, from the UN-FLOORED albedo means:
 *                   da = max(max(|a_r(p) - a_r(q)|, |a_g(p) - a_g(q)|), |a_b(p) - a_b(q)|)
 *                   y = da / sigma_albedo;  ta = 1 - y * y;  ea = (ta > 0 ? ta * ta : 0)
 *                   w = (h[dy] * h[dx]) * (e * ea)
 *              sw, sc, sv, C_k+1 and V_k+1 as there                (sw >= 9/64 still: the centre tap has e = ea = 1)
 *   Output.    d_mean_out_c = C_K,c * d_c for a valid pixel (m_c for any other); d_rgba8, if not NULL, the bytes rt_resolve_rgba8_device
 *              gives for d_mean_out, written by the last iteration itself.
 * With A_c = n_a everywhere (and albedo_floor <= 1), d = 1, I = m, u = v, ea = 1, e * 1 = e and C * 1 = C, each exactly: the result is
 * rt_denoise_device's bit for bit. */
typedef struct rt_denoise_albedo_params {
    uint32_t struct_size;   /* sizeof(rt_denoise_albedo_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t iterations;     /* K, 1..6 (default 4): strides 1, 2, 4, ... 2^(K-1) */
    double sigma;           /* as rt_denoise_params (default 4.0), > 0 */
    double eps;             /* as rt_denoise_params (default 1e-6), > 0 */
    double sigma_albedo;    /* width of the albedo stop: a tap whose albedo differs by this much or more in any channel has weight 0
                               (default 0.5), > 0 */
    double albedo_floor;    /* the smallest divisor (default 1e-3), > 0 */
} rt_denoise_albedo_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_denoise_albedo_params_init_sized(rt_denoise_albedo_params *params, uint32_t struct_size);
/* Bytes of device memory rt_denoise_albedo_device needs for a w x h frame (the two halves of rt_denoise_device and the guide: three
 * regions of 4 doubles per pixel); -1 for a size it refuses. */
int64_t rt_denoise_albedo_workspace_bytes(int32_t width, int32_t height);
int rt_denoise_albedo_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp,
                             const int32_t *d_spp /* NULL: uniform spp */, const double *d_albedo_sum /* 3*w*h */,
                             int32_t albedo_spp /* >= 1 */, const rt_denoise_albedo_params *params /* NULL: defaults */,
                             double *d_mean_out /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);

/* ---- surface-ID scene and edge-guided denoise (opt-in; nothing above changes) ------------------------------------------------------------
 * Neither filter above can stop at a GEOMETRIC edge between two surfaces of one colour: the luminance stop sees only the noisy frame, and
 * the albedo frame of a white box in front of a white wall is flat.  A per-pixel "which surface did the first hit land on" frame can,
 * and it needs no new render path either: it is an ordinary render of the SURFACE-ID SCENE of a description.
 *
 * Surface-ID scene.  The same geometry with every primitive and every medium given one of RT_SURFACE_ID_COLOURS palette colours, as a
 * DIFFUSE_LIGHT of a SOLID texture.  As in an albedo scene a light does not scatter, and the camera's and the media's draws come before
 * a material's: path (seed, p, s) of the ID scene ends at the first hit of path (seed, p, s) of the original and returns that surface's
 * colour — lens, shutter and the random hit inside a constant medium included — so the frame is anti-aliased by the beauty frame's own
 * samples.  Normative rule (rt_surface_id_tables):
 *   Palette entry q, 1 <= q <= 26, is the colour (0.5 * (q % 3), 0.5 * ((q / 3) % 3), 0.5 * (q / 9)) in integer arithmetic: every
 *   channel is 0, 0.5 or 1, each exactly representable, and black (q = 0) is not in the palette.  Two different entries differ by at
 *   least 0.5 in some channel.
 *   out_textures[i], i = 0 .. 25, is {kind SOLID, even = odd = image = perlin = -1, _pad 0, color = palette entry i + 1, inv_scale 0,
 *   scale 0};  out_materials[i] is {DIFFUSE_LIGHT, texture i, albedo, fuzz and ir zero}.
 *   Surfaces are numbered k = 0, 1, ... in this order: spheres in array order, then quads, then media.  Surface k uses material k % 26,
 *   so any 26 consecutive surfaces of a description get distinct colours.
 *   out_spheres and out_quads are copies of desc->spheres and desc->quads with only `material` rewritten; out_media are copies of
 *   desc->media with only `phase_material` rewritten.  The description's own materials and textures are not read.
 * rt_surface_id_tables touches no device.  RT_ERR_INVALID_ARGUMENT (the message names the field), in this order: a null desc,
 * out_spheres, out_quads, out_media, out_materials or out_textures (each is required even where its count is 0); abi_version other
 * than RT_ABI_VERSION; a negative n_spheres, n_quads or n_media, or a null spheres / quads / media array with a non-zero count.
 * Nothing is written then.
 * rt_scene_create_surface_ids is rt_scene_create_ex on `desc` with those five tables and n_materials = n_textures = 26 swapped in:
 * everything else — lists, transforms, trees, options — is the caller's.  Every texture of an ID scene is a SOLID, so it is rendered
 * by the kernel class of its geometry with solid textures, whatever the original's textures were (an image- or noise-textured original
 * is rendered by another kernel than its ID scene).
 * The caller's CAMERA decides what a miss contributes.  The layers above this ABI render the ID scene with the beauty camera and
 * background = (0, 0, 0): black is no palette colour, so the background is a surface of its own to the filter below. */
#define RT_SURFACE_ID_COLOURS 26
int rt_surface_id_tables(const rt_scene_desc *desc, rt_sphere *out_spheres /* desc->n_spheres */, rt_quad *out_quads /* desc->n_quads */,
                         rt_constant_medium *out_media /* desc->n_media */, rt_material *out_materials /* RT_SURFACE_ID_COLOURS */,
                         rt_texture *out_textures /* RT_SURFACE_ID_COLOURS */);
int rt_scene_create_surface_ids(const rt_scene_desc *desc, int device, const rt_scene_options *options /* NULL: defaults */,
                                rt_scene **out_scene);

/* rt_denoise_guided_device is rt_denoise_albedo_device — or, with d_albedo_sum NULL, rt_denoise_device — with an EDGE GUIDE beside
 * its inputs: d_edge_sum holds 3 * w * h doubles, the per-pixel sums of edge_spp samples of a guide frame (a surface-ID scene's render,
 * an albedo scene's, or any other frame whose edges the filter should respect).  An edge guide contributes one stop factor per tap and
 * nothing else: nothing is divided by it and nothing is multiplied back in.  The contract is the other filters': enqueued on
 * hip_stream, not synchronised, nothing allocated; d_workspace is rt_denoise_guided_workspace_bytes(w, h, d_albedo_sum != NULL) bytes
 * of device memory, 16-byte aligned.  With d_albedo_sum NULL, albedo_spp, sigma_albedo and albedo_floor are not read.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: width or height < 1 or w * h >= 2^27; a null d_sum,
 * d_sum_sq, d_edge_sum, d_mean_out or d_workspace; spp < 2 when d_spp is NULL; with an albedo frame, albedo_spp < 1; edge_spp < 1; a
 * struct_size this library does not know; iterations outside 1..6; sigma or eps that is not a number > 0; with an albedo frame, a
 * sigma_albedo or albedo_floor that is not a number > 0; a sigma_edge that is not a number > 0; d_mean_out overlapping d_sum, d_sum_sq
 * or d_albedo_sum; d_mean_out overlapping d_edge_sum; a d_rgba8 that is not 4-byte aligned; a d_workspace that is not 16-byte aligned.
 *
 * Normative definition.  Everything is as in rt_denoise_albedo_device (with d_albedo_sum NULL: as in rt_denoise_device), f64 with every
 * operation rounded on its own, with these additions; E is p's entry of d_edge_sum and n_e = edge_spp as a double:
 *   Prepare.   g_c = E_c / n_e.  A VALID pixel also needs all three E_c finite.  C0 and V0 are what they are without the edge guide.
 *   Iteration. One more factor per tap:
 *                   dg = max(max(|g_r(p) - g_r(q)|, |g_g(p) - g_g(q)|), |g_b(p) - g_b(q)|)
 *                   z = dg / sigma_edge;  tg = 1 - z * z;  eg = (tg > 0 ? tg * tg : 0)
 *                   w = (h[dy] * h[dx]) * ((e * ea) * eg)   with an albedo frame,   w = (h[dy] * h[dx]) * (e * eg)   without
 *              (sw >= 9/64 still: the centre tap has eg = 1)
 *   Output.    As without the edge guide: it is not multiplied in.
 * With E_c the same value at every pixel, dg = 0, z = 0, tg = 1, eg = 1 and x * 1 = x, each exactly: the result is
 * rt_denoise_albedo_device's (rt_denoise_device's) bit for bit.  The means (live), spatial-variance and views forms of this call are rt_denoise_guided_mean_device,
 * rt_denoise_guided_mean_spatial_device and rt_denoise_guided_views_device: "edge guide on every route" below. */
typedef struct rt_denoise_guided_params {
    uint32_t struct_size;   /* sizeof(rt_denoise_guided_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t iterations;     /* K, 1..6 (default 4): strides 1, 2, 4, ... 2^(K-1) */
    double sigma;           /* as rt_denoise_params (default 4.0), > 0 */
    double eps;             /* as rt_denoise_params (default 1e-6), > 0 */
    double sigma_albedo;    /* as rt_denoise_albedo_params (default 0.5), > 0; read only with an albedo frame */
    double albedo_floor;    /* as rt_denoise_albedo_params (default 1e-3), > 0; read only with an albedo frame */
    double sigma_edge;      /* width of the edge guide's stop: a tap whose guide differs by this much or more in any channel has weight 0
                               (default 0.5: two surface-ID colours differ by at least that), > 0 */
} rt_denoise_guided_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_denoise_guided_params_init_sized(rt_denoise_guided_params *params, uint32_t struct_size);
/* Bytes of device memory rt_denoise_guided_device needs for a w x h frame: the two halves and the edge guide's region, and with
 * with_albedo != 0 the albedo guide's as well (three or four regions of 4 doubles per pixel); -1 for a size it refuses. */
int64_t rt_denoise_guided_workspace_bytes(int32_t width, int32_t height, int32_t with_albedo);
int rt_denoise_guided_device(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp,
                             const int32_t *d_spp /* NULL: uniform spp */, const double *d_albedo_sum /* 3*w*h, or NULL: no albedo guide */,
                             int32_t albedo_spp /* >= 1 with an albedo frame */, const double *d_edge_sum /* 3*w*h */,
                             int32_t edge_spp /* >= 1 */, const rt_denoise_guided_params *params /* NULL: defaults */,
                             double *d_mean_out /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);

/* ---- live denoise: a running second moment beside the running mean, and the filters on (mean, M2) (opt-in; nothing above changes) ----
 * Live refinement shows the noisiest frames there are — 1, 2, 3 ... samples per pixel — and a running mean keeps no second moment, so
 * neither filter above can take its frame.  These calls close that gap: a reduction that keeps Welford's M2 beside the mean, and a
 * means-form input for the two filters.
 *
 * rt_render_mean_moments_device is rt_render_mean_device with a second frame of 3 * w * h doubles, d_m2.  Per channel, f64, every
 * operation rounded on its own (no FMA, IEEE division):
 *     for s = sample_begin .. sample_end - 1:
 *         d  = c_s - m
 *         m' = m + d / (double)(s + 1)            (rt_render_mean_device's recurrence, word for word)
 *         M2 = M2 + d * (c_s - m')                (the product rounded, then added)
 *         m  = m'
 * sample_begin == 0 starts m and M2 from +0.0 and reads neither buffer; any other sample_begin continues both, so [0, a) followed by
 * [a, b) equals [0, b) bit for bit.  d_mean is, bit for bit, what rt_render_mean_device writes, and d_rgba8 follows its contract (the
 * call's last launch writes it, in the same pass).  m' lies between m and c_s, so d and c_s - m' have one sign or are zero: every term is
 * >= 0, M2 never decreases and is never negative, and a pixel whose samples are all equal has M2 = +0.0 exactly — none of which holds
 * for Q - S * m.  M2 / (n - 1) is the sample variance after n samples.  Limits and refusals are rt_render_mean_device's, and a null
 * d_m2 / m2: RT_ERR_INVALID_ARGUMENT with the field named, before the scene handle or any device work is touched.
 * rt_render_mean_moments blocks and downloads; when sample_begin > 0 it uploads `mean` and `m2` first.
 *
 * rt_denoise_mean_device and rt_denoise_albedo_mean_device are rt_denoise_device and rt_denoise_albedo_device on such frames: d_mean
 * and d_m2 (3 * w * h doubles each) after `samples` samples of every pixel — the count is uniform, there is no map — and, guided,
 * d_albedo_mean, the frame rt_render_mean_device gives for the albedo scene.  Workspaces are rt_denoise_workspace_bytes and
 * rt_denoise_albedo_workspace_bytes.  Only Prepare differs; with n = (double)samples and m, M2, a the pixel's entries:
 *   Prepare.   p is VALID iff samples >= 2 and every m_c and M2_c (guided: and a_c) is finite.  For a valid pixel
 *              v_c = M2_c / (n - 1)
 *              V0 = max(max(max(v_r, v_g), v_b), 0) / n;   C0 = m
 *              guided:  d_c = max(a_c, albedo_floor)  (a is not divided);  C0 = m / d;  u_c = v_c / (d_c * d_c) in v_c's place.
 *              A pixel that is not valid keeps C = m, is written to the output unchanged and is never a tap: with samples < 2 the whole
 *              output is d_mean, bit for bit.  Any M2 may be passed, a negative one too: the max(.., 0) covers it.
 *   Iterations and Output: those of rt_denoise_device / rt_denoise_albedo_device, unchanged (guided: the stop reads the un-floored a).
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, as the sums forms give it: width or height < 1 or w * h >= 2^27; a
 * null d_mean, d_m2, d_albedo_mean, d_mean_out or d_workspace; samples < 1; a struct_size this library does not know; iterations
 * outside 1..6; sigma, eps, sigma_albedo or albedo_floor that is not a number > 0; d_mean_out overlapping an input; a d_rgba8 that is
 * not 4-byte aligned. */
int rt_render_mean_moments_device(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                                  double *d_mean /* 3*w*h */, double *d_m2 /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */,
                                  void *hip_stream);
int rt_render_mean_moments(const rt_scene *scene, const rt_camera *camera, const rt_render_params *params,
                           double *mean /* host; read when sample_begin > 0 */, double *m2 /* host; likewise */,
                           uint8_t *rgba8 /* host, or NULL */);
int rt_denoise_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                           const rt_denoise_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h */,
                           uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int rt_denoise_albedo_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                  const double *d_albedo_mean /* 3*w*h */, const rt_denoise_albedo_params *params /* NULL: defaults */,
                                  double *d_mean_out /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace,
                                  void *hip_stream);

/* ---- spatial variance: the means-form filters on frames of too few samples for M2 (opt-in; nothing above changes) ---------------------
 * The means forms above call a pixel valid only from two samples on, so the first live frame — and every frame of a caller who restarts
 * the mean on each camera move — leaves them unfiltered.  These calls estimate the variance of such a frame from the spread of the
 * neighbouring pixels' values instead of from each pixel's own samples (SVGF's fallback for pixels with a short history).
 *
 * rt_denoise_mean_spatial_device and rt_denoise_albedo_mean_spatial_device take the means forms' arguments and an
 * rt_denoise_spatial_params (NULL: defaults).  With samples >= spatial_below the call IS rt_denoise_mean_device /
 * rt_denoise_albedo_mean_device: the same kernels, bit for bit, and d_m2 is required.  With samples < spatial_below the spatial Prepare
 * below runs in the means forms' place; d_m2 is not read and may be NULL.  spatial_below = 1 never takes the spatial route.  The contract
 * is the means forms': enqueued on hip_stream, not synchronised, nothing allocated; the workspaces are rt_denoise_workspace_bytes and
 * rt_denoise_albedo_workspace_bytes.
 *
 * Normative definition.  The arithmetic is that of "denoise": f64 throughout, every operation rounded on its own (no FMA, IEEE
 * division), max(a, b) = (b > a ? b : a).  m, a are the pixel's entries of d_mean, d_albedo_mean; R = window_radius.
 *   Prepare.   p is VALID iff every m_c (guided: and every a_c) is finite; d_m2 is not read.
 *              C0 = m;  guided:  d_c = max(a_c, albedo_floor),  C0_c = m_c / d_c  (the guide written is the un-floored a, as above).
 *              A pixel that is not valid keeps C = m and V = -1, is written to the output unchanged and is never a tap or a window member.
 *              For a valid p the window is q = p + (dx, dy), dy = -R..R outer, dx = -R..R inner, over the in-frame valid pixels; p itself
 *              is a member.  cnt is the number of members, as a double.  Per channel, in that order:
 *                   s1_c = +0.0;  s1_c = s1_c + C0_c(q)  for every member;          mu_c = s1_c / cnt
 *                   s2_c = +0.0;  t = C0_c(q) - mu_c;  s2_c = s2_c + t * t          (the product rounded, then added)
 *                   v_c = s2_c / (cnt - 1)  where cnt >= 2, else +0.0
 *              V0 = max(max(v_r, v_g), v_b).  Nothing is divided by n: the window's values already are n-sample means, so their spread
 *              estimates the variance of a mean (plus the signal's own variation).  V0 >= 0 by construction.  On a window whose
 *              members all equal c it is +0.0 exactly wherever the in-order sums 2c, 3c, .. cnt * c are exact — any c of at most 47
 *              significant bits, the window having at most 49 members — since then mu = c; for any other c, mu may miss c by rounding
 *              and V0 is a residue of at most 2 * (cnt * 2^-52 * |c|)^2.
 *   Iterations and Output: those of rt_denoise_device / rt_denoise_albedo_device, unchanged.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in the means forms' order with the new checks behind `samples`:
 * everything the means forms refuse (a null d_m2 only as below); an rt_denoise_spatial_params.struct_size this library does not know;
 * spatial_below < 1; window_radius outside 1..3; a null d_m2 when samples >= spatial_below. */
typedef struct rt_denoise_spatial_params {
    uint32_t struct_size;   /* sizeof(rt_denoise_spatial_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t spatial_below;  /* the spatial estimate serves frames of fewer samples than this (default 2: where M2 has nothing), >= 1 */
    int32_t window_radius;  /* R, 1..3 (default 1): the window is (2R + 1) x (2R + 1) pixels */
} rt_denoise_spatial_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_denoise_spatial_params_init_sized(rt_denoise_spatial_params *params, uint32_t struct_size);
int rt_denoise_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2 /* or NULL, see above */,
                                   int32_t samples, const rt_denoise_spatial_params *spatial /* NULL: defaults */,
                                   const rt_denoise_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h */,
                                   uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int rt_denoise_albedo_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2 /* or NULL, see above */,
                                          int32_t samples, const double *d_albedo_mean /* 3*w*h */,
                                          const rt_denoise_spatial_params *spatial /* NULL: defaults */,
                                          const rt_denoise_albedo_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h */,
                                          uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);

/* ---- views moments: sums and sums of squares per view (opt-in; nothing above changes) ---------------------------------------------------
 * Views mode renders many small frames of few samples in one launch, and those are the frames that most need the filters above; these
 * calls give them the second moment the filters read, without giving up the single job space.
 *
 * rt_render_views_moments_device is rt_render_views_device with a second buffer: d_sum and d_sum_sq each hold n_views frames of
 * 3 * w * h doubles, view-major.  Checks, limits and the launch path are rt_render_views_device's.
 *   d_sum       is, bit for bit, what rt_render_views_device writes.
 *   d_sum_sq[v] is, bit for bit, what rt_render_moments_device writes as d_sum_sq under (views[v].camera, seed = views[v].seed): per
 *               channel the in-order sum of each sample's c * c, the product rounded and then added, with no contraction.
 * params->accumulate continues both buffers; without it neither buffer's previous content is read.  A call that is cut into several
 * launches gives one launch's bits in both buffers.  Padding pixels of edge tiles are not written, and nothing behind the last view is.
 * A null d_sum_sq is refused with RT_ERR_INVALID_ARGUMENT (the field named) before any device work: callers who want no squares have
 * rt_render_views_device.  rt_render_views_moments blocks and downloads; with accumulate set it uploads both buffers first. */
int rt_render_views_moments_device(const rt_scene *scene, const rt_view *views /* HOST, n_views entries, copied */, int32_t n_views,
                                   const rt_render_params *params, double *d_sum /* n_views frames of 3*w*h doubles, view-major */,
                                   double *d_sum_sq /* likewise */, void *hip_stream);
int rt_render_views_moments(const rt_scene *scene, const rt_view *views, int32_t n_views, const rt_render_params *params,
                            double *sum /* host */, double *sum_sq /* host */);

/* ---- views denoise: one filter over a stack of frames (opt-in; nothing above changes) ---------------------------------------------------
 * rt_denoise_device takes one frame per call, K + 1 launches each, and at the sizes views mode serves those launches are what it costs.
 * rt_denoise_views_device and rt_denoise_albedo_views_device are rt_denoise_device and rt_denoise_albedo_device over n_views frames
 * in the same K + 1 launches, whatever n_views is.  Every frame pointer is view-major: d_sum, d_sum_sq, d_albedo_sum and d_mean_out
 * hold n_views frames of 3 * w * h doubles, d_rgba8 n_views frames of 4 * w * h bytes.  spp is uniform (the views share their sample
 * range: there is no map on this route).  d_workspace is rt_denoise_views_workspace_bytes(w, h, n_views) or
 * rt_denoise_albedo_views_workspace_bytes(w, h, n_views) bytes, 16-byte aligned: n_views times the single-frame figure, or -1 for what
 * the call would refuse or what overflows.  Enqueued on hip_stream, not synchronised, nothing allocated.
 *
 * Normative.  View v of d_mean_out (and of d_rgba8) is, bit for bit, what the single-frame entry point gives for view v's frames with
 * the same parameters.  A tap, a halo pixel or a member of the 3 x 3 variance window that lies outside view v's own w x h frame is out
 * of frame: it is never a pixel of view v - 1 or v + 1, although those lie adjacent in memory.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in the single-frame order with n_views behind the frame size:
 * everything rt_denoise_device / rt_denoise_albedo_device refuses (spp < 2 always: there is no map); n_views < 1; n_views >
 * RT_DENOISE_MAX_VIEWS (the view is the second dimension of the launch grid, which carries 65535 at most); d_mean_out overlapping an
 * input anywhere in the whole n_views extent.  The means forms and the spatial-variance form have no views form: there is no live
 * views route for them to serve. */
#define RT_DENOISE_MAX_VIEWS 65535
int64_t rt_denoise_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views);
int64_t rt_denoise_albedo_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views);
int rt_denoise_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                            const rt_denoise_params *params /* NULL: defaults */, double *d_mean_out /* n_views x 3*w*h */,
                            uint8_t *d_rgba8 /* n_views x 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int rt_denoise_albedo_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const double *d_albedo_sum /* n_views x 3*w*h */, int32_t albedo_spp /* >= 1 */,
                                   const rt_denoise_albedo_params *params /* NULL: defaults */, double *d_mean_out /* n_views x 3*w*h */,
                                   uint8_t *d_rgba8 /* n_views x 4*w*h, or NULL */, void *d_workspace, void *hip_stream);

/* ---- edge guide on every route: the means, spatial-variance and views forms of rt_denoise_guided_device (opt-in; nothing above changes) ----
 * The edge guide of rt_denoise_guided_device on the three other routes of the filter.  All three take rt_denoise_guided_params (NULL:
 * defaults; struct_size as everywhere) and an optional albedo frame: with it NULL, albedo_spp, sigma_albedo and albedo_floor are not
 * read and the call is the plain form's with an edge guide.  Each is enqueued on hip_stream, not synchronised, and allocates nothing;
 * d_workspace is 16-byte aligned.
 *
 * rt_denoise_guided_mean_device is rt_denoise_albedo_mean_device (d_albedo_mean NULL: rt_denoise_mean_device) with an edge guide.
 * d_edge_mean holds 3 * w * h doubles, a frame of MEANS — what rt_render_mean_device gives for the surface-ID scene — so there is no
 * count.  d_workspace is rt_denoise_guided_workspace_bytes(w, h, d_albedo_mean != NULL) bytes.  Normative, as "live denoise" with:
 *   Prepare.   g_c = E_c, nothing divided (as a is not).  A VALID pixel also needs all three E_c finite.  C0 and V0 are untouched.
 *   Iterations and Output: rt_denoise_guided_device's.
 * With samples < 2 the output is d_mean bit for bit.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: width or height < 1 or w * h >= 2^27; a null d_mean,
 * d_m2, d_edge_mean, d_mean_out or d_workspace; samples < 1; a struct_size this library does not know; iterations outside 1..6; sigma
 * or eps that is not a number > 0; with an albedo frame, a sigma_albedo or albedo_floor that is not a number > 0; a sigma_edge that is
 * not a number > 0; d_mean_out overlapping d_mean, d_m2 or d_albedo_mean; d_mean_out overlapping d_edge_mean; a d_rgba8 that is not
 * 4-byte aligned; a d_workspace that is not 16-byte aligned.
 *
 * rt_denoise_guided_mean_spatial_device is rt_denoise_albedo_mean_spatial_device (rt_denoise_mean_spatial_device) with an edge guide.
 * With samples >= spatial_below the call IS rt_denoise_guided_mean_device: the same kernels, d_m2 required.  Below it an EDGE-AWARE
 * spatial Prepare runs and d_m2 is not read and may be NULL.  The workspace is rt_denoise_guided_mean_device's.  Normative, as "spatial
 * variance" (f64, every operation rounded on its own, max(a, b) = (b > a ? b : a)) with g = E, the pixel's entry of d_edge_mean:
 *   Prepare.   p is VALID iff every m_c is finite, with an albedo frame every a_c is finite, and every E_c is finite.
 *              For a valid p and an in-frame valid q of the (2R + 1)^2 window, dy outer and dx inner:
 *                   dg = max(max(|g_r(p) - g_r(q)|, |g_g(p) - g_g(q)|), |g_b(p) - g_b(q)|)
 *                   z = dg / sigma_edge;  tg = 1 - z * z;  q is a MEMBER iff tg > 0
 *              (the iterations' edge stop is non-zero exactly there).  p is a member of its own window: dg = 0.  cnt, s1, mu, s2, v_c
 *              and V0 are "spatial variance"'s over the members, and nothing else changes.  The albedo stop does not decide
 *              membership: demodulation already took the albedo out of C0.  The guide of an out-of-frame or invalid pixel is never
 *              read.  The edge region is written (g = E), and with an albedo frame the albedo region as there.
 *   Iterations and Output: rt_denoise_guided_device's.
 * With E the same at every pixel every valid window pixel is a member, and the result is the unguided spatial form's bit for bit.
 * With samples < 2 and no spatial route (spatial_below = 1) the output is d_mean bit for bit.
 * RT_ERR_INVALID_ARGUMENT, in rt_denoise_guided_mean_device's order with the spatial checks behind `samples`: width or height < 1 or
 * w * h >= 2^27; a null d_mean, d_edge_mean, d_mean_out or d_workspace; samples < 1; an rt_denoise_spatial_params.struct_size this
 * library does not know; spatial_below < 1; window_radius outside 1..3; a null d_m2 when samples >= spatial_below; then everything
 * from "a struct_size this library does not know" on as above.
 *
 * rt_denoise_guided_views_device is rt_denoise_albedo_views_device (d_albedo_sum NULL: rt_denoise_views_device) with an edge guide,
 * view-major everywhere: d_sum, d_sum_sq, d_albedo_sum, d_edge_sum and d_mean_out hold n_views frames of 3 * w * h doubles, d_rgba8
 * n_views frames of 4 * w * h bytes.  View v of d_mean_out (and of d_rgba8) is, bit for bit, rt_denoise_guided_device on view v's
 * frames; no tap, halo pixel or window member is another view's.  d_workspace is rt_denoise_guided_views_workspace_bytes(w, h, n_views,
 * d_albedo_sum != NULL) bytes: n_views times rt_denoise_guided_workspace_bytes, or -1 for what the call refuses or what overflows.
 * RT_ERR_INVALID_ARGUMENT, in this order: width or height < 1 or w * h >= 2^27; n_views < 1; n_views > RT_DENOISE_MAX_VIEWS; a null
 * d_sum, d_sum_sq, d_edge_sum, d_mean_out or d_workspace; spp < 2; with an albedo frame, albedo_spp < 1; edge_spp < 1; a struct_size
 * this library does not know; iterations outside 1..6; sigma or eps that is not a number > 0; with an albedo frame, a sigma_albedo or
 * albedo_floor that is not a number > 0; a sigma_edge that is not a number > 0; d_mean_out overlapping d_sum, d_sum_sq or d_albedo_sum
 * anywhere in the whole n_views extent; d_mean_out overlapping d_edge_sum likewise; a d_rgba8 that is not 4-byte aligned; a
 * d_workspace that is not 16-byte aligned. */
int rt_denoise_guided_mean_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                  const double *d_albedo_mean /* 3*w*h, or NULL: no albedo guide */, const double *d_edge_mean /* 3*w*h */,
                                  const rt_denoise_guided_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h */,
                                  uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int rt_denoise_guided_mean_spatial_device(int32_t width, int32_t height, const double *d_mean, const double *d_m2 /* or NULL, see above */,
                                          int32_t samples, const double *d_albedo_mean /* 3*w*h, or NULL: no albedo guide */,
                                          const double *d_edge_mean /* 3*w*h */, const rt_denoise_spatial_params *spatial /* NULL: defaults */,
                                          const rt_denoise_guided_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h */,
                                          uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);
int64_t rt_denoise_guided_views_workspace_bytes(int32_t width, int32_t height, int32_t n_views, int32_t with_albedo);
int rt_denoise_guided_views_device(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const double *d_albedo_sum /* n_views x 3*w*h, or NULL: no albedo guide */,
                                   int32_t albedo_spp /* >= 1 with an albedo frame */, const double *d_edge_sum /* n_views x 3*w*h */,
                                   int32_t edge_spp /* >= 1 */, const rt_denoise_guided_params *params /* NULL: defaults */,
                                   double *d_mean_out /* n_views x 3*w*h */, uint8_t *d_rgba8 /* n_views x 4*w*h, or NULL */,
                                   void *d_workspace, void *hip_stream);

/* ---- guided upsampling (opt-in; nothing above changes) -------------------------------------------------------------------------------------
 * A frame's cost is its number of paths.  Where a picture is wanted quickly, trace the beauty frame at 1/F of the width and height —
 * 1/F^2 of the paths — and bring it to full size with a joint bilateral upsampler that takes its EDGES from a full-size surface-ID
 * frame and its TEXTURE DETAIL from a full-size albedo frame, both first-hit renders of about one bounce per sample: irradiance is
 * interpolated between the low pixels, stopped where the guides differ, and the albedo is multiplied back per full-size pixel.
 *
 * rt_camera_scaled gives the camera of the small frame.  F = factor, 2, 3 or 4; lw = (w + F - 1) / F and lh = (h + F - 1) / F in integer
 * arithmetic.  *out is *camera with image_width = lw, image_height = lh, and per component, every operation rounded on its own,
 *      du' = F * du;   dv' = F * dv                               (du = pixel_delta_u, dv = pixel_delta_v; F as a double)
 *      pixel00_loc' = (pixel00_loc - (0.5 * (du + dv))) + (0.5 * (du' + dv'))
 * so that low pixel (I, J) covers exactly the full-size pixels [F I, F I + F) x [F J, F J + F); where F does not divide the size the
 * last low column or row reaches past the frame.  Lens, background, depth and spp are untouched; out may be camera.  No device is
 * touched.  RT_ERR_INVALID_ARGUMENT, in this order: a null camera; a null out; a factor outside 2..4.
 *
 * Normative definition of rt_upsample_device.  f64, every operation rounded on its own, no FMA, IEEE division;
 * max(a, b) = (b > a ? b : a).  (x, y) is a full-size pixel, index y * w + x; (I, J) a low pixel, index J * lw + I.  S is a low
 * pixel's entry of d_low, A and E a full-size pixel's entries of d_albedo_sum and d_edge_sum; n_a = albedo_spp, n_e = edge_spp as doubles.
 *   Low values.   C_c = S_c * (1.0 / (double)spp).
 *   Full guides.  a_c(p) = A_c / n_a;  g_c(p) = E_c / n_e                            (each only where that guide is given)
 *   Low guides.   For each guide given, the mean of the guide's full-size means over the IN-FRAME pixels of the low pixel's F x F block:
 *                 acc = +0.0; for y = F J .. F J + F - 1 (y < h) outer, x = F I .. F I + F - 1 (x < w) inner: acc_c = acc_c + a_c(x, y);
 *                 a_low_c = acc_c / (double)count, count the number of pixels added.  g_low likewise.
 *                 A low pixel is VALID iff its three C_c and, for each guide given, its three low guide values are finite.
 *                 With an albedo guide  d_c = max(a_low_c, albedo_floor);  R_c = C_c / d_c.   Without one  R = C.
 *   Footprint.    t = 2 x + 1 - F;  i0 = floor(t / (2 F)) (integer floor division: t is negative in the first columns);
 *                 rx = t - 2 F i0, in [0, 2 F).  The same in y gives j0 and ry.  Taps: J = j0 - 1 .. j0 + 2 outer, I = i0 - 1 .. i0 + 2
 *                 inner; a tap outside the low frame or not VALID is skipped.
 *                 ax = |2 F (I - i0) - rx| (an integer, at most 4 F);  wx = (double)(4 F - ax) / (double)(4 F) >= 0 — a tent of two low pixels'
 *                 radius about the full-size pixel's centre; exact for F = 2 and 4, one rounded division for F = 3.  For F = 3, t is even and
 *                 rx can be 0: the tap I = i0 + 2 then has ax = 4 F and weight +0.0, and adds nothing.  wy likewise;  ws = wy * wx.
 *   Stops.        The denoisers' stops between the FULL guide at p = (x, y) and the LOW guide at the tap q:
 *                      dg = max(max(|g_r(p) - g_low_r(q)|, |g_g(p) - g_low_g(q)|), |g_b(p) - g_low_b(q)|)
 *                      z = dg / sigma_edge;  tg = 1 - z * z;  eg = (tg > 0 ? tg * tg : 0)
 *                 and ea the same from a(p), a_low(q) (both un-floored) and sigma_albedo.
 *                      w = ws * (ea * eg)  with both guides;  w = ws * ea,  w = ws * eg  with one;  w = ws  with none
 *                      sw = sw + w;   sc_c = sc_c + (w * R_c(q))                       (both from +0.0)
 *   Output.       sw > 0:  r_c = sc_c / sw.   Otherwise (every tap outside, invalid or stopped):  r = R of the containing low pixel
 *                 (x / F, y / F) as it is, valid or not.
 *                 out_c = r_c * max(a_c(p), albedo_floor) with an albedo guide, out = r without.  d_mean_out holds out; d_rgba8, if not
 *                 NULL, the bytes rt_resolve_rgba8_device gives for out, written by the same kernel.
 * A non-finite low pixel is never a tap, so it shows at most in its own block (where every other tap is stopped too) and nowhere else;
 * a non-finite guide pixel makes its own block's low pixel invalid and stops every tap of its own, and spreads no further.
 * Consequences.  With no guide and a low frame of one dyadic value, F = 2 or 4: every weight is dyadic and out is that value bit for
 * bit.  A guide that is the same at every pixel changes nothing against no guide (dg = 0, eg = 1, x * 1 = x, each exactly; an albedo
 * guide of A = n_a everywhere and albedo_floor <= 1 likewise: d = 1, R = C, ea = 1, r * 1 = r).  A full-size pixel whose in-frame,
 * valid taps all carry its own guide values takes the plain tent result.
 *
 * rt_upsample_device takes the FULL size.  It reads d_low (3 * lw * lh doubles: sums with the count spp, or means with spp = 1) and
 * the guides given, and writes d_mean_out (3 * w * h doubles) and, if given, d_rgba8 (4 * w * h bytes); no input is written.  It works
 * in d_workspace (rt_upsample_workspace_bytes(w, h, factor) bytes of device memory, 16-byte aligned, the caller's; nothing in it is read
 * before the call writes it).  The call is enqueued on hip_stream, does not synchronise and allocates nothing.  Without a guide its spp
 * and its sigma are not used.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1; w * h >= 2^27; a null d_low, d_mean_out
 * or d_workspace; spp < 1; an albedo guide with albedo_spp < 1; an edge guide with edge_spp < 1; a struct_size this library does not
 * know; a factor outside 2..4; sigma_edge, sigma_albedo or albedo_floor that is not a number > 0 (checked whichever guides are given); a
 * d_rgba8 that is not 4-byte aligned; a d_workspace that is not 16-byte aligned; d_mean_out overlapping d_low, d_albedo_sum or
 * d_edge_sum. */
int rt_camera_scaled(const rt_camera *camera, int32_t factor, rt_camera *out);
typedef struct rt_upsample_params {
    uint32_t struct_size;   /* sizeof(rt_upsample_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t factor;         /* F, 2..4 (default 2): the low frame is ceil(w / F) x ceil(h / F) */
    double sigma_edge;      /* width of the edge guide's stop (default 0.5: two surface-ID colours differ by at least that), > 0 */
    double sigma_albedo;    /* width of the albedo guide's stop (default 0.5), > 0 */
    double albedo_floor;    /* the smallest divisor and factor (default 1e-3), > 0 */
} rt_upsample_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_upsample_params_init_sized(rt_upsample_params *params, uint32_t struct_size);
/* Bytes of device memory the call needs for a FULL size of w x h at this factor (three regions — R with the valid flag, the low albedo
 * and the low edge guide — of 4 doubles per LOW pixel); -1 for a size or a factor the call refuses. */
int64_t rt_upsample_workspace_bytes(int32_t width, int32_t height, int32_t factor);
int rt_upsample_device(int32_t width, int32_t height /* the FULL size */, const double *d_low /* 3*lw*lh */,
                       int32_t spp /* sums with a count; means: 1 */, const double *d_albedo_sum /* 3*w*h, or NULL */, int32_t albedo_spp,
                       const double *d_edge_sum /* 3*w*h, or NULL */, int32_t edge_spp, const rt_upsample_params *params /* NULL: defaults */,
                       double *d_mean_out /* 3*w*h */, uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace, void *hip_stream);

/* ---- robust frames (opt-in; nothing above changes) ---------------------------------------------------------------------------------------
 * Every route above ends in the plain mean of a pixel's samples, which has no defence against a firefly: one rare path that carries
 * hundreds of times the pixel's settled value stays a white dot at 4 to 64 samples, and the filters and bloom behind it keep or spread
 * the dot.  rt_robust_device is the median of means: a pixel's samples arrive as K independent BLOCKS — K sub-frames of one camera under
 * seeds seed + k, which rt_render_views_device renders in one launch — and the K block means are combined by a trimmed mean whose trim
 * grows from 0 (the ordinary mean) to the median as the block means become more unequal.
 *
 * Normative definition.  The arithmetic rules are those of "Arithmetic" below: f64, every operation rounded on its own, no FMA, IEEE
 * division.  The input is a block-major stack of K = blocks frames of 3 * w * h doubles, d_stack[k * 3wh + (j*w + i)*3 + c] — what
 * rt_render_views_device writes — of sums with the uniform per-block count spp, or of means with spp = 1.  Each of the 3 * w * h values
 * is treated on its own; a pixel's channels never meet.
 *   Input value.  mu_k = S_k * (1.0 / (double)spp), tone mapping's "Input value"; a mu_k that is a NaN is replaced by THE NaN, the bit
 *                 pattern 0x7ff8000000000000, so that all NaNs of a value are one.
 *   Order.        mu_(0) .. mu_(K-1) are the K values sorted ascending; THE NaN sorts behind +inf; -0.0 and +0.0 compare equal.  Values
 *                 that compare equal differ at most in a zero's sign, and every sum below starts from +0.0, where a zero of either sign
 *                 adds the same: the order among equal values cannot change a result bit.
 *   Trim count.   tmax = (K - 1) / 2 (integer division: the median for odd K, the two central values for even K), and by mode
 *                   RT_ROBUST_MEAN    t = 0
 *                   RT_ROBUST_TRIM    t = min(trim, tmax)
 *                   RT_ROBUST_MEDIAN  t = tmax
 *                   RT_ROBUST_GINI    if any mu_k is not finite, t = tmax.  Otherwise
 *                                       S = the sum of mu_(i), W = the sum of ((double)(2*i - K + 1)) * mu_(i) (the product rounded, then
 *                                       added), both over i = 0 .. K-1 in order from +0.0;
 *                                       if S > 0 and W > 0:  g = (gain * (W / S)) * 0.5;  t = (int32_t)g if g < (double)tmax, else tmax
 *                                       (so also for a g that is no number); otherwise t = 0.
 *                 In exact arithmetic W / (K * S) is the Gini coefficient G of the block means, so g = gain * G * K / 2: equal blocks
 *                 give W = 0 and t = 0, and one block that holds everything gives W / S = K - 1, which at gain 1 is the median.
 *   Output.       If mu_(t) == mu_(K-1-t) — the kept values are all equal, and no NaN — out = mu_(t) + 0.0 (the value itself; a zero of
 *                 either sign leaves as +0.0).  Otherwise m = K - 2*t;  acc = +0.0;  for i = t .. K-1-t in order: acc = acc + mu_(i);
 *                 out = acc / (double)m, THE NaN if a NaN.  (A sum of m equal values need not divide back to the value unless m is a
 *                 power of two; the first rule keeps a constant pixel constant at any K.)
 *   M2 (optional) the winsorised second moment: w_i = mu_(t) for i < t, mu_(K-1-t) for i > K-1-t, mu_(i) otherwise;
 *                 M2 = the sum over i = 0 .. K-1 in order from +0.0 of (w_i - out) * (w_i - out) (the difference rounded, the product
 *                 rounded, then added), THE NaN if a NaN.  With samples = K, (out, M2) is what rt_denoise_mean_device reads: its Prepare
 *                 forms M2 / (K - 1) / K, the variance of the combined mean.  M2 is >= +0.0 or THE NaN, never negative.
 * Consequences.  K = 1: out = mu_0 (a -0.0 leaves as +0.0) and M2 = +0.0 for a finite mu_0.  RT_ROBUST_MEAN is the SORTED-order mean of
 * the block means: it is not rt_render's sum over the samples in their order and need not equal it to the bit; on K copies of one frame
 * every mode gives that frame's means exactly.  Where all blocks of a value are equal and finite, M2 = +0.0.  With t >= 1, raising
 * the t largest values of a pixel to anything larger, +inf and NaN included, or lowering the t smallest, changes no bit of out as long as
 * t stays what it was — under RT_ROBUST_TRIM and RT_ROBUST_MEDIAN t does not depend on the values; under RT_ROBUST_GINI it does, and a
 * value that stops being finite makes it tmax.  A NaN or +inf in at most t blocks does not reach out.
 *
 * rt_robust_device reads d_stack and writes d_mean_out (3 * w * h doubles of means) and, if it is not NULL, d_m2_out (likewise); with
 * or without d_m2_out, d_mean_out gets the same bits.  One launch, enqueued on hip_stream; the call does not synchronise, allocates
 * nothing and has no workspace.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; blocks outside
 * 1..RT_ROBUST_MAX_BLOCKS; a null d_stack or d_mean_out; spp < 1; a struct_size this library does not know; mode outside 0..3; trim < 0;
 * gain that is not a finite number > 0; d_mean_out overlapping any of the stack's `blocks` frames, d_m2_out likewise, d_m2_out
 * overlapping d_mean_out. */
#define RT_ROBUST_MAX_BLOCKS 32
#define RT_ROBUST_MEAN 0
#define RT_ROBUST_TRIM 1
#define RT_ROBUST_MEDIAN 2
#define RT_ROBUST_GINI 3
typedef struct rt_robust_params {
    uint32_t struct_size;   /* sizeof(rt_robust_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t mode;           /* RT_ROBUST_* (default RT_ROBUST_GINI) */
    int32_t trim;           /* RT_ROBUST_TRIM only: >= 0, clamped to tmax (default 1) */
    double gain;            /* RT_ROBUST_GINI only: finite, > 0 (default 1.0) */
} rt_robust_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_robust_params_init_sized(rt_robust_params *params, uint32_t struct_size);
int rt_robust_device(int32_t width, int32_t height, int32_t blocks, const double *d_stack /* blocks x 3*w*h, block-major */, int32_t spp,
                     const rt_robust_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h MEANS */,
                     double *d_m2_out /* 3*w*h, or NULL */, void *hip_stream);

/* ---- bloom (opt-in; nothing above changes) ------------------------------------------------------------------------------------------------
 * A tone curve works one pixel at a time: a radiance-15 lamp and a radiance-1.5 wall beside it both end near white.  rt_bloom_device
 * spreads the light of the pixels above a luminance threshold over their neighbourhood BEFORE the curve: a bright pass, K levels of the
 * separable five-tap B3-spline blur at strides 1, 2, 4, ... (the a-trous scheme of the denoisers: a glow of radius 2 * (2^K - 1) pixels at
 * full resolution, ten taps per level, no resampling), the levels' average added back to the frame.  Its output is a frame of MEANS: feed
 * it to rt_tonemap_device with spp = 1, or to rt_resolve_rgba8_device.
 *
 * Normative definition.  The arithmetic rules are those of "Arithmetic" below: f64, every operation rounded on its own, no FMA, IEEE
 * division.  h = (1/16, 1/4, 3/8, 1/4, 1/16), indexed by d = -2 .. 2; pixel (i, j) has index j * w + i.
 *   Input value.  m_c = S_c * (1.0 / (double)n), exactly tone mapping's "Input value" (n = spp, or d_spp[pixel]; means form: spp == 1,
 *                 no map).
 *   Bright pass.  L = ((0.2126 * m_r) + (0.7152 * m_g)) + (0.0722 * m_b).
 *                 p is BRIGHT iff all three m_c are finite, L is finite and L > threshold.
 *                 Bright:  k = (L - threshold) / L;  B0_c = m_c * k.     Any other pixel: B0_c = +0.0.
 *                 (threshold == 0: k = L / L = 1 exactly, B0 = m.)
 *   Level k = 0 .. K-1, stride s = 2^k, per channel:
 *      H_c(i,j)     = acc, where acc = +0.0; for d = -2 .. 2 in order, skipping i + s*d outside [0, w):
 *                         acc = acc + (h[d] * B_k,c(i + s*d, j))
 *      B_k+1,c(i,j) = the same along j over H_c (skipping j + s*d outside [0, h))
 *      A_k+1,c      = A_k,c + B_k+1,c              (A_0 = +0.0)
 *   Output.       g_c = A_K,c / (double)K;  out_c = m_c + (strength * g_c)     for EVERY pixel, bright or not.
 * Taps outside the frame are skipped and nothing is renormalised: light that leaves the frame is lost.  A non-finite pixel is never a
 * source, so NaN and +-inf do not spread; such a pixel keeps its own m through the final addition.
 * Consequences.  If no pixel is bright, g = +0.0 and out = m (bit for bit on a frame without -0.0): followed by rt_tonemap_device with
 * the clamp, exposure 1 and no key, the bytes are those of rt_resolve_rgb8_device, rt_resolve_rgb8_spp_device and rt_resolve_rgba8_device.
 * A single bright pixel of value 1 with threshold 0, far from the border, gives the outer products of h exactly: all weights are dyadic.
 *
 * rt_bloom_device reads d_values (3 * w * h doubles: sums with the uniform count spp or the per-pixel map d_spp, or means with spp = 1)
 * and writes d_mean_out (3 * w * h doubles); d_values is not written.  It works in d_workspace (rt_bloom_workspace_bytes(w, h) bytes of
 * device memory, 16-byte aligned, the caller's; nothing in it is read before the call writes it).  The call is enqueued on hip_stream,
 * does not synchronise and allocates nothing.  spp must be >= 1 even where d_spp is given (it is then not read).  There is no views form:
 * a stack of views is blurred one view per call, because a tap must never leave its own frame.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; a null d_values,
 * d_mean_out or d_workspace; spp < 1; a struct_size this library does not know; levels outside 1..8; threshold that is not a finite
 * number >= 0; strength likewise; a d_workspace that is not 16-byte aligned; d_mean_out overlapping d_values. */
typedef struct rt_bloom_params {
    uint32_t struct_size;   /* sizeof(rt_bloom_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t levels;         /* K, 1..8 (default 5): strides 1 .. 2^(K-1) */
    double threshold;       /* luminance above which a pixel is a source: finite, >= 0 (default 1.0) */
    double strength;        /* factor of the glow added back: finite, >= 0 (default 0.25) */
} rt_bloom_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_bloom_params_init_sized(rt_bloom_params *params, uint32_t struct_size);
/* Bytes of device memory the call needs for a w x h frame (three regions — B, H and A — of 24 * w * h bytes, each rounded up to a
 * multiple of 16); -1 for a size the call refuses. */
int64_t rt_bloom_workspace_bytes(int32_t width, int32_t height);
int rt_bloom_device(int32_t width, int32_t height, const double *d_values /* 3*w*h */, int32_t spp, const int32_t *d_spp /* NULL: uniform */,
                    const rt_bloom_params *params /* NULL: defaults */, double *d_mean_out /* 3*w*h MEANS */, void *d_workspace,
                    void *hip_stream);

/* ---- tone mapping (opt-in; nothing above changes) ----------------------------------------------------------------------------------------
 * Every route above ends in color_to_rgb: (u8)(256 * clamp(x^(1/2.2), 0, 0.999)).  Radiance above 1 is clipped flat and a dark frame
 * cannot be lifted.  rt_tonemap_device is that output stage with an exposure and a tone curve in front of the gamma, and optionally an
 * automatic exposure from the frame's log-average luminance, reduced on the device: the call never synchronises with the host.
 *
 * Normative definition.  The arithmetic rules are those of "Arithmetic" below: f64, every operation rounded on its own, no FMA, IEEE
 * division.
 *   Input value.  Sums form: m = S * (1.0 / (double)n), the multiplication by the reciprocal that rt_resolve_rgb8_device and
 *                 rt_resolve_rgb8_spp_device do; n is spp, or d_spp[pixel].  Means form (spp == 1, no map): m = S * 1.0 = S.
 *   Exposure.     x = m * scale, with scale = exposure when auto_key == 0.  exposure is a linear factor (the layers above this ABI
 *                 convert stops with exp2).
 *   Operator.     Per channel, applied only where 0 < x < +inf; any other x (zero, negative, NaN, +-inf) passes through unchanged, so
 *                 rt_gamma_encode / rt_quantise treat it as they do in the stages above.
 *                   RT_TONEMAP_CLAMP:     y = x
 *                   RT_TONEMAP_REINHARD:  w2 = white * white;  r = x / w2;  r = 1 + r;  num = x * r;  den = 1 + x;  y = num / den
 *                                         (white = +inf is allowed and is the default: r is then exactly 1 and y = x / (1 + x))
 *                   RT_TONEMAP_ACES:      a = 2.51 * x;  a = a + 0.03;  num = x * a;
 *                                         b = 2.43 * x;  b = b + 0.59;  den = x * b;  den = den + 0.14;  y = num / den   (Narkowicz's fit)
 *   Bytes.        rt_quantise(rt_gamma_encode(y)) per value (d_rgb8, 3 * w * h bytes); d_rgba8 packs a pixel's three bytes as
 *                 rt_resolve_rgba8_device does, with alpha 0xff, in one 32-bit store.
 *   With RT_TONEMAP_CLAMP, exposure == 1 and auto_key == 0 every step is exact (x * 1.0 == x): the bytes are exactly those of
 *   rt_resolve_rgb8_device, rt_resolve_rgb8_spp_device and rt_resolve_rgba8_device.
 *   Auto-exposure (auto_key > 0; Reinhard's log-average).  Per pixel p, in index order j * w + i:
 *                 L = ((0.2126 * m_r) + (0.7152 * m_g)) + (0.0722 * m_b).  p COUNTS iff all three m_c are finite and L >= 0.  A counting
 *                 pixel has the term t_p = rt_log(delta + L) (the fixed ln of "Arithmetic"); any other pixel the term +0.0 and count 0.
 *                 Reduction, in a fixed order: the terms are padded to a multiple of 256 with +0.0 and count 0; each block of 256
 *                 consecutive entries is reduced by the tree
 *                     for stride = 128, 64, ..., 1:   e[i] = e[i] + e[i + stride]   for i < stride
 *                 (counts are integers); the block results, in block order, are the entries of the next level; levels repeat until one
 *                 entry (T, count) is left — at most four levels below 2^27 pixels.  Then
 *                     log_mean = T / (double)count;  Lavg = rt_exp(log_mean);  scale = exposure * (auto_key / Lavg)
 *                 and with count == 0: scale = exposure, log_mean = Lavg = 0.
 *                 The tree is normative: no floating-point atomics, and no summation order that depends on the launch shape.
 *
 * rt_tonemap_device reads d_values (3 * w * h doubles: sums with the uniform count spp or the per-pixel map d_spp, or means with spp = 1)
 * and writes d_rgb8, d_rgba8 or both; d_values is not written.  With auto_key > 0 it runs the reduction first, in d_workspace
 * (rt_tonemap_workspace_bytes(w, h) bytes of device memory, 16-byte aligned, the caller's), whose first four doubles are afterwards
 * log_mean, Lavg, (double)count and scale; the value kernels read scale from there.  rt_log_average_luminance_device is the reduction
 * alone: it writes log_mean, Lavg, (double)count and 0 to d_out4 (device memory).  Both calls are enqueued on hip_stream, do not
 * synchronise and allocate nothing.  spp must be >= 1 even where d_spp is given (it is then not read).
 * With auto_key == 0 the call is elementwise: a stack of n_views frames is a frame of height n_views * h.  Auto-exposure over such a
 * frame would pool the views into one log-average; callers who want one exposure per view call once per view.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; a null d_values; both
 * outputs null (rt_log_average_luminance_device: a null d_out4); spp < 1; a struct_size this library does not know; op outside 0..2;
 * exposure that is not a finite number > 0; delta likewise; auto_key that is not a finite number >= 0; white that is not > 0 (+inf
 * allowed); with auto_key > 0 (rt_log_average_luminance_device: always) a null d_workspace or one that is not 16-byte aligned; a
 * d_rgba8 that is not 4-byte aligned; an output overlapping d_values. */
#define RT_TONEMAP_CLAMP 0
#define RT_TONEMAP_REINHARD 1
#define RT_TONEMAP_ACES 2
typedef struct rt_tonemap_params {
    uint32_t struct_size;   /* sizeof(rt_tonemap_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t op;             /* RT_TONEMAP_* (default RT_TONEMAP_CLAMP) */
    double exposure;        /* linear factor (default 1.0), finite, > 0 */
    double auto_key;        /* 0: off (default); > 0: the key the log-average luminance is mapped to (the layers above: 0.18) */
    double delta;           /* added to the luminance inside the logarithm (default 1e-4), finite, > 0 */
    double white;           /* Reinhard: the value that maps to 1 (default +inf), > 0 */
} rt_tonemap_params;
/* Fills the defaults into the first struct_size bytes (nothing beyond them is written) and sets struct_size. */
int rt_tonemap_params_init_sized(rt_tonemap_params *params, uint32_t struct_size);
/* Bytes of device memory the reduction needs for a w x h frame (four doubles of results and 16 bytes per block of every level);
 * -1 for a size the calls refuse. */
int64_t rt_tonemap_workspace_bytes(int32_t width, int32_t height);
int rt_tonemap_device(int32_t width, int32_t height, const double *d_values /* 3*w*h */, int32_t spp, const int32_t *d_spp /* NULL: uniform */,
                      const rt_tonemap_params *params /* NULL: defaults */, uint8_t *d_rgb8 /* 3*w*h, or NULL */,
                      uint8_t *d_rgba8 /* 4*w*h, or NULL */, void *d_workspace /* may be NULL when auto_key == 0 */, void *hip_stream);
int rt_log_average_luminance_device(int32_t width, int32_t height, const double *d_values /* 3*w*h */, int32_t spp,
                                    const int32_t *d_spp /* NULL: uniform */, double delta, double *d_out4 /* log_mean, Lavg, count, 0 */,
                                    void *d_workspace, void *hip_stream);

/* ---- film output (opt-in; nothing above changes) -------------------------------------------------------------------------------------------
 * Every stage above ends in eight-bit gamma bytes.  rt_film_device is the tone-mapping stage with another last step: the value the stage
 * would gamma-encode and quantise is written in a format that keeps it — the shared-exponent pixels of a Radiance .hdr file, floats for
 * a PFM, or sixteen-bit gamma samples for a PNG — so that radiance above 1 leaves the device unclipped in 4 or 12 bytes per pixel
 * instead of the sums' 24.
 *
 * Normative definition.  d_values, spp and d_spp are tone mapping's, and so is the value before encoding, bit for bit:
 *     m = tone mapping's "Input value";  x = m * scale;  y = rt_tonemap(op, x, w2)
 * with scale = exposure, or with auto_key > 0 the scale of tone mapping's "Auto-exposure": the same reduction tree in the same workspace
 * (rt_tonemap_workspace_bytes), whose first four doubles are afterwards log_mean, Lavg, (double)count and scale.  With the defaults
 * (clamp, exposure 1, no key) y == m exactly: the linear formats then hold the frame's radiance.
 *   RT_FILM_RGBE   4 bytes per pixel, Radiance's shared exponent (Ward's float2rgbe with its one inexact step, m * 256 / v, made exact),
 *                  one 32-bit store per pixel, R in the lowest byte as rt_resolve_rgba8_device packs, the exponent byte on top.
 *                  Per channel c = y where y > 0 (+inf included), else c = 0: zero, negatives and NaN give 0.  c = min(c, 255 * 2^119),
 *                  the largest value the format holds.  v = max(c_r, c_g, c_b).  v < 2^-128: the pixel is 0, 0, 0, 0.  Otherwise e is the
 *                  integer with 2^(e-1) <= v < 2^e, taken from the exponent field of v's bits (v is normal here; no library frexp);
 *                  b_k = (uint8_t)(c_k * 2^(8-e)), an exact multiplication by a power of two built from bits, then truncated;
 *                  E = e + 128, in 1..255.  Hence b_k * 2^(E-136) <= c_k < (b_k + 1) * 2^(E-136), and the largest byte is >= 128.
 *   RT_FILM_F32    3 floats per pixel: y rounded to f32, to nearest, ties to even.  Overflow gives +-inf, signs are kept, values below
 *                  f32's normal range become f32 subnormals or +-0, and every NaN becomes the one bit pattern 0x7fc00000.
 *   RT_FILM_RGB16  3 native-endian uint16_t per pixel: g = rt_gamma_encode(y); NaN gives 0, otherwise
 *                  (uint16_t)(65536.0 * clamp(g, 0, 0.99999)).  The high byte of every value is the byte rt_tonemap_device writes for the
 *                  same input and params: the scalings by 256 and 65536 are exact and both clamps land in 255.
 *
 * rt_film_device reads d_values and writes rt_film_bytes(w, h, format) bytes at d_out; d_values is not written.  The call is enqueued
 * on hip_stream, does not synchronise and allocates nothing.  rt_film_bytes is w * h * (4, 12 or 6); -1 for a frame or a format the
 * call refuses.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; a null d_values; a
 * null d_out; spp < 1; format outside 0..2; the rt_tonemap_params checks of tone mapping, in its order; with auto_key > 0 a null
 * d_workspace or one that is not 16-byte aligned; a d_out that is not 4-byte aligned (RT_FILM_RGB16: 2-byte); d_out overlapping
 * d_values. */
#define RT_FILM_RGBE 0
#define RT_FILM_F32 1
#define RT_FILM_RGB16 2
int64_t rt_film_bytes(int32_t width, int32_t height, int32_t format);
int rt_film_device(int32_t width, int32_t height, const double *d_values /* 3*w*h */, int32_t spp, const int32_t *d_spp /* NULL: uniform */,
                   const rt_tonemap_params *tone /* NULL: defaults */, int32_t format /* RT_FILM_* */, void *d_out /* rt_film_bytes */,
                   void *d_workspace /* may be NULL when auto_key == 0 */, void *hip_stream);

/* ---- panoramas (opt-in; nothing above changes) ----------------------------------------------------------------------------------------------
 * A full 360 x 180 degree picture of a scene from one point: the six faces of a cube map are six views of ONE rt_render_views_device
 * launch, and rt_panorama_device resamples them into an equirectangular frame of means, which bloom, tone mapping and the film stage
 * take as any frame of means (spp = 1) — the equirectangular .hdr is what viewers and image-based lighting read.
 *
 * Cube-face cameras.  rt_camera_cube_faces (no device) fills six square pinhole cameras of F = face_size pixels (defocus_angle 0, both
 * disk vectors 0) centred at `center` (NULL: like->center); samples_per_pixel, max_depth and background are like's.  The inner
 * (F - 2 g)^2 texels of a face (g = guard) cover exactly 90 degrees and the g texels around them continue the same grid outwards, so
 * with g >= 1 a bilinear tap near a seam stays inside its own face and reads what the neighbouring face would show.  World axes, +Y up,
 * right = forward x up (the reference camera's vup x w):
 *       face   forward n   up u   right r
 *        0       +X         +Y     +Z
 *        1       -X         +Y     -Z
 *        2       +Y         +Z     +X
 *        3       -Y         -Z     +X
 *        4       +Z         +Y     -X
 *        5       -Z         +Y     +X
 *   Plain f64, each operation rounded on its own, no trigonometry and no normalisation:
 *       delta = 2.0 / (double)(F - 2 g);   hh = (double)F / (double)(F - 2 g);   e = 0.5 * delta - hh
 *       pixel_delta_u = r * delta;   pixel_delta_v = u * (-delta)          (every component is +-delta or 0)
 *       pixel00_loc_c = center_c + t_c,  t = n + r * e - u * e              (three different axes: every t_c is exactly one of +-1, +-e)
 *   so that texel (i, j) of a face looks along n + r * ((2 i + 1 - F) / (F - 2 g)) - u * ((2 j + 1 - F) / (F - 2 g)).
 *   RT_ERR_INVALID_ARGUMENT (the field named), in this order: a null like or out; face_size outside 2..16384; guard < 0;
 *   face_size - 2 * guard < 1.
 *
 * Tables.  rt_panorama_tables (no device) writes 2 w + 2 h doubles to HOST memory, column entries first, then row entries:
 *       tables[2 i]       = sin(lambda_i),  tables[2 i + 1]       = cos(lambda_i),   lambda_i = (((double)i + 0.5) / (double)w - 0.5) * 2 pi
 *       tables[2 w + 2 j] = sin(phi_j),     tables[2 w + 2 j + 1] = cos(phi_j),      phi_j = (0.5 - ((double)j + 0.5) / (double)h) * pi
 *   for the rows j with 2 j < h; row h - 1 - j is its mirror image (-sin(phi_j), cos(phi_j)), so the two hemispheres are each other's
 *   reflection to the bit (the formula itself rounds differently above and below the equator).  The centre column looks along -Z, the
 *   reference camera's default direction; longitude grows towards +X; row 0 is up.  The tables are DATA the caller uploads once per
 *   size, and the only place a transcendental enters (the host's libm): the kernel and the host mirror read the same tables, so their
 *   outputs agree bit for bit whatever libm made them.  The resampler does not require them to be normalised.
 *   RT_ERR_INVALID_ARGUMENT: w or h < 1, or w * h >= 2^27; a null tables.
 *
 * The resampler, normative definition.  The arithmetic rules are those of "Arithmetic" below: f64, every operation rounded on its own,
 * no FMA, IEEE division.  d_faces are six frames of 3 F F doubles, face-major — what rt_render_views_device writes for the six cameras
 * above — of sums with the uniform count spp, or of means with spp = 1.  Per output pixel (i, j), with (sl, cl) column i's entries and
 * (sp, cp) row j's:
 *   Direction.    dx = cp * sl;  dy = sp;  dz = -(cp * cl).
 *   Face.         ax, ay, az the absolute values.  ax >= ay and ax >= az: face 0 if dx > 0, else 1, m = ax.  Else ay >= az: face 2 if
 *                 dy > 0, else 3, m = ay.  Otherwise face 4 if dz > 0, else 5, m = az.  Ties go to X over Y over Z.
 *   Face coords.  a = (d . r) / m;  b = (d . u) / m — each dot product is one signed component of d, exact, so |a|, |b| <= 1.
 *   Texel coords. s = (double)(F - 2 g) * 0.5;  c = (double)F * 0.5 - 0.5;  x = a * s + c;  y = c - b * s;
 *                 x0 = min(max((int32_t)floor(x), 0), F - 2);  fx = min(max(x - (double)x0, 0.0), 1.0);  y0 and fy likewise.
 *                 With g >= 1 no clamp ever acts; with g = 0 they are clamp-to-edge.
 *   Taps.         T = S * (1.0 / (double)spp), tone mapping's "Input value", at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
 *                 of the chosen face: T00, T10, T01, T11.
 *   Output.       Per channel:  top = T00 + (T10 - T00) * fx;  bot = T01 + (T11 - T01) * fx;  out = top + (bot - top) * fy.
 * Consequences.  A stack of one finite value gives that value bit for bit (every difference is +0.0).  A non-finite texel reaches
 * exactly the output pixels that tap it, also at weight 0 (0 * inf and 0 * NaN are NaN), and no other.  With g = 2 the outermost texel
 * ring of every face is never read: |a| <= 1 puts x in [g - 0.5, F - g - 0.5], whose taps are columns g - 1 .. F - g.
 *
 * rt_panorama_device reads d_tables (2 w + 2 h doubles, DEVICE memory) and d_faces and writes d_mean_out (3 w h doubles of means); no
 * input is written.  One launch, enqueued on hip_stream; the call does not synchronise, allocates nothing and has no workspace.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; face_size and guard
 * as rt_camera_cube_faces refuses them; a null d_tables, d_faces or d_mean_out; spp < 1; d_mean_out overlapping d_tables or any of
 * the six faces. */
int rt_camera_cube_faces(const rt_camera *like, const double center[3] /* NULL: like->center */, int32_t face_size, int32_t guard,
                         rt_camera out[6]);
int rt_panorama_tables(int32_t width, int32_t height, double *tables /* HOST, 2*width + 2*height doubles */);
int rt_panorama_device(int32_t width, int32_t height, const double *d_tables /* 2w + 2h, device */,
                       const double *d_faces /* 6 frames of 3*F*F doubles, face-major */, int32_t face_size, int32_t guard,
                       int32_t spp /* sums with a count; means: 1 */, double *d_mean_out /* 3*w*h MEANS */, void *hip_stream);

/* ---- frame metrics (opt-in; nothing above changes) -------------------------------------------------------------------------------------------
 * How good is a frame?  rt_frame_error_device measures a frame against a reference frame of the same size (MSE, relative MSE, mean
 * absolute error, bias, largest error, PSNR); rt_frame_noise_device estimates a frame's own noise from its second moments, so that a
 * refining loop can stop when the picture has settled.  Both are one reduction over the pixels, on the device, without a host round trip.
 *
 * Normative definition.  The arithmetic rules are those of "Arithmetic" below: f64, every operation rounded on its own, no FMA, IEEE
 * division and square root, rt_log where a logarithm is needed.  max(a, b) = (a < b ? b : a).
 *   Reduction.    Exactly tone mapping's tree: one entry per pixel in index order j * w + i, padded to a multiple of 256 with the
 *                 neutral entry; each block of 256 consecutive entries is reduced by
 *                     for stride = 128, 64, ..., 1:   e[i] = e[i] (+) e[i + stride]   for i < stride
 *                 the block results, in block order, are the entries of the next level; levels repeat until one entry is left.  An
 *                 entry is a record of several accumulators: (+) adds sums, takes max of maxima and adds the integer counts.  The
 *                 neutral entry is all +0.0 with count 0.  No floating-point atomics, and no summation order that depends on the
 *                 launch shape.  w * h < 2^27, as there.
 *   Input value.  As in "tone mapping".  Sums form: m = S * (1.0 / (double)n), n uniform or d_spp[pixel].  Means form: m = S.
 *
 * rt_frame_error_device.  d_values is a frame of sums with the count spp or the map d_spp, or of means with spp = 1; d_ref a frame of
 * sums with the uniform count ref_spp, or of means with ref_spp = 1: r = R * (1.0 / (double)ref_spp).
 *   Counting.     A pixel COUNTS iff its three m and three r are all finite.  Any other pixel is the neutral entry.
 *   Per channel of a counting pixel.   d = m - r;  sq = d * d;  ab = |d|;  den = (r * r) + eps;  rel = sq / den.
 *   Pixel entry.  T_sq, T_rel, T_ab, T_d: (t_r + t_g) + t_b of sq, rel, ab and d;  Tmax = max(max(ab_r, ab_g), ab_b);  count 1.
 *   Final values, with N = (double)(3 * count), written to d_out8 in this order:
 *                 count (as a double);  mse = T_sq / N;  rmse = sqrt(mse);  rel_mse = T_rel / N;  mae = T_ab / N;  bias = T_d / N;
 *                 max_abs = Tmax;  psnr = 4.342944819032518 * rt_log((peak * peak) / mse)  (the constant is 10 / ln 10), and +inf where
 *                 mse == 0.  With count == 0 all eight are 0.
 *
 * rt_frame_noise_device.  form RT_METRICS_SUMS: d_a holds per-pixel sums S and d_b sums of squares Q (rt_render_moments_device), with
 * the count n or the map d_spp.  form RT_METRICS_MEANS: d_a holds the running means and d_b Welford's M2 after n samples of every
 * pixel (rt_render_mean_moments_device); uniform n only.
 *   Counting.     A pixel COUNTS iff its n >= 2 and its six values are finite.  Any other pixel is the neutral entry.
 *   Variance.     Per channel, with dn = (double)n, the variance of the mean as the denoisers' Prepare step has it before it takes the
 *                 largest channel — "denoise": m_c = S_c / dn, v_c = (Q_c - S_c * m_c) / (dn - 1); "live denoise": v_c = M2_c / (dn - 1) —
 *                 then var_c = (0 > v_c ? 0 : v_c) / dn.  The largest var_c of a pixel is Prepare's V0 bit for bit.
 *   Per channel.  mean = the "Input value" above;  rel = var / ((mean * mean) + eps).
 *   Pixel entry.  V = (var_r + var_g) + var_b;  R = (rel_r + rel_g) + rel_b;  Rmax = max(max(rel_r, rel_g), rel_b);  count 1.
 *   Final values, with N = (double)(3 * count), written to d_out4 in this order:
 *                 count (as a double);  mean_var = V / N;  noise = sqrt(R / N), the RMS relative standard error;
 *                 max_noise = sqrt(Rmax).  With count == 0: mean_var = 0 and noise = max_noise = +inf, so that a test
 *                 `noise <= threshold` never passes on a frame that says nothing (every pixel at n = 1).
 *
 * Both calls read their inputs and write only the output doubles (DEVICE memory) and d_workspace: rt_metrics_workspace_bytes(w, h)
 * bytes of device memory, 16-byte aligned, the caller's — 48 bytes per block of every level; -1 for a size the calls refuse.  They are
 * enqueued on hip_stream, do not synchronise and allocate nothing.  spp / n must be >= 1 even where d_spp is given (it is then not read).
 * The entries of d_spp are the caller's to keep >= 1, as in "tone mapping": they are not checked.  An entry of 0 makes 1.0 / 0 = +inf, so the
 * error call's m is +-inf or NaN and the pixel does not count; a negative entry negates m, and the pixel counts with it; in the noise call
 * an entry below 2 does not count.
 * RT_ERR_INVALID_ARGUMENT (the field named) before any device work, in this order: w or h < 1, or w * h >= 2^27; a null d_values,
 * d_ref, d_out8 (d_a, d_b, d_out4); spp < 1, ref_spp < 1 (n < 1); a struct_size this library does not know; form outside 0..1, or a
 * d_spp map with RT_METRICS_MEANS; eps (and peak) that is not a finite number > 0; a null d_workspace or one that is not 16-byte
 * aligned; the output overlapping an input frame. */
#define RT_METRICS_SUMS 0
#define RT_METRICS_MEANS 1
typedef struct rt_frame_error_params {
    uint32_t struct_size;   /* sizeof(rt_frame_error_params) as the CALLER was compiled (grows like rt_scene_options) */
    int32_t _pad;
    double eps;             /* added to the squared reference in rel's denominator (default 1e-2), finite, > 0 */
    double peak;            /* the signal peak of psnr (default 1.0), finite, > 0 */
} rt_frame_error_params;
typedef struct rt_frame_noise_params {
    uint32_t struct_size;   /* sizeof(rt_frame_noise_params) as the CALLER was compiled */
    int32_t _pad;
    double eps;             /* added to the squared mean in rel's denominator (default 1e-2), finite, > 0 */
} rt_frame_noise_params;
/* Fill the defaults into the first struct_size bytes (nothing beyond them is written) and set struct_size. */
int rt_frame_error_params_init_sized(rt_frame_error_params *params, uint32_t struct_size);
int rt_frame_noise_params_init_sized(rt_frame_noise_params *params, uint32_t struct_size);
int64_t rt_metrics_workspace_bytes(int32_t width, int32_t height);
int rt_frame_error_device(int32_t width, int32_t height, const double *d_values /* 3*w*h */, int32_t spp, const int32_t *d_spp /* NULL: uniform */,
                          const double *d_ref /* 3*w*h */, int32_t ref_spp, const rt_frame_error_params *params /* NULL: defaults */,
                          double *d_out8 /* count, mse, rmse, rel_mse, mae, bias, max_abs, psnr */, void *d_workspace, void *hip_stream);
int rt_frame_noise_device(int32_t width, int32_t height, int32_t form /* RT_METRICS_* */, const double *d_a /* 3*w*h */,
                          const double *d_b /* 3*w*h */, int32_t n, const int32_t *d_spp /* NULL: uniform; sums form only */,
                          const rt_frame_noise_params *params /* NULL: defaults */, double *d_out4 /* count, mean_var, noise, max_noise */,
                          void *d_workspace, void *hip_stream);

/* Device memory for hosts that do not link the HIP runtime themselves (the Rust binding, host/renderer.cpp): the buffers
 * rt_render_device, the gather and the frame-end kernels work on.  rt_device_download copies to host memory and returns when
 * the copy — and everything enqueued on hip_stream before it — is done; rt_device_upload is the other direction (small inputs such as
 * rt_panorama_tables' doubles) and returns when the host memory may be reused. */
int rt_device_malloc(int device, int64_t bytes, void **out_device_ptr);
int rt_device_free(int device, void *device_ptr);
int rt_device_download(int device, void *dst_host, const void *src_device, int64_t bytes, void *hip_stream);
int rt_device_upload(int device, void *dst_device, const void *src_host, int64_t bytes, void *hip_stream);

/* ---- frame-end gather over RCCL / xGMI ----------------------------------------------------------
 * One communicator handle per rank (= per GPU).  Create it either
 *   - one process per GPU: rank 0 calls rt_comm_get_unique_id and hands the 128 bytes to the other ranks by whatever
 *     channel the host program has (MPI, a file, a socket); every rank then calls rt_comm_create;
 *   - one process, several GPUs: rt_comm_create_all (ncclCommInitAll), then one thread per device;
 *   - or wrap a communicator the host already owns: rt_comm_adopt(ncclComm_t).
 * rt_gather_tiles_device brings every rank's RT_OUT_TILES buffer (f64 sums: elem_bytes 8; resolved RGB8: elem_bytes 1)
 * to `root` in ONE grouped exchange (N - 1 receives on the root, one send per other rank, each on its own xGMI link) into
 * d_gathered = [rank 0's tiles | rank 1's | ...], every slot rt_out_size(w, h, RT_OUT_TILES, 0, N) elements long — the
 * layout rt_tiles_to_frame_device / rt_tiles_to_frame_rgb8_device take.  d_gathered is only read on the root.
 * Enqueued on hip_stream; RCCL is loaded on first use (RT_ERR_COMM if it is not installed). */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm; /* opaque */
int rt_comm_get_unique_id(uint8_t out_id[RT_COMM_ID_BYTES]);
int rt_comm_create(const uint8_t id[RT_COMM_ID_BYTES], int rank, int n_ranks, int device, rt_comm **out_comm);
int rt_comm_create_all(int n_devices, const int *devices /* NULL: 0 .. n-1 */, rt_comm **out_comms /* [n_devices] */);
int rt_comm_adopt(void *nccl_comm, int device, rt_comm **out_comm);
void rt_comm_destroy(rt_comm *comm);
int rt_comm_rank(const rt_comm *comm);
int rt_comm_size(const rt_comm *comm);
int rt_gather_tiles_device(rt_comm *comm, int32_t width, int32_t height, int32_t elem_bytes, const void *d_tiles,
                           void *d_gathered, int root, void *hip_stream);

const char *rt_last_error(void);
const char *rt_version(void);

/* ---- Normative definitions shared by every implementation of this ABI ------------------------------
 *
 * RNG.  The reference draws from rand 0.8.5's thread_rng(), which is OS-seeded and cannot be reproduced
 * (Cargo.toml:10; call sites src/vec3.rs:43-50,:80-81, src/camera.rs:123,:134-135, src/material.rs:94,
 * src/constant_medium.rs:48).  This ABI replaces it by a seeded generator with one stream per camera path, so
 * that an image is a pure function of (scene, camera, seed):
 *
 *     mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     key(seed, pixel, sample) = mix64( mix64(seed + 0x9E3779B97F4A7C15) ^ ((u64)pixel << 32 | (u32)sample) )
 *     stream of that path (RomuDuoJr): x = key, y = mix64(key + 0x9E3779B97F4A7C15); every draw returns x and then
 *         (x, y) <- (0xD3833E804F4C574B * y,  rotl64(y - x, 27))                  (all arithmetic mod 2^64)
 *     (round 1 used one splitmix64 output per draw: two 64-bit multiplies; this form needs one — DESIGN.md "RNG")
 *
 * pixel = j * image_width + i (src/renderer.rs:32-33); sample counts from 0.  The draws of one camera path
 * are consumed in the reference's program order (camera px, py, [disk x, y]*, time; then per bounce the
 * draws of ConstantMedium::hit in traversal order, then the material's).  From a 64-bit draw x:
 *
 *     random::<f64>()        = (x >> 11) * 2^-53                               (rand 0.8 Standard for f64)
 *     gen_range(lo..hi)      = (f64::from_bits((x >> 12) | 0x3FF0000000000000) - 1.0) * (hi - lo) + lo
 *                                                                               (rand 0.8 UniformFloat::sample_single)
 *
 * Arithmetic.  IEEE-754 binary64, round-to-nearest-even, no fused multiply-add contraction, operations in
 * the reference's source order.  Square root and division are correctly rounded.  The five transcendental
 * functions on the path — ln (src/constant_medium.rs:48), sin (src/texture.rs:109), acos and atan2
 * (src/sphere.rs:49-50), x^5 (src/material.rs:77) — are computed by the fixed algorithms documented in
 * DESIGN.md ("Device math") so that CPU and GPU implementations agree bit for bit; they are within 2 ulp
 * of a correctly rounded result (x^5: 3 ulp).  gamma_to_linear on texels (src/color.rs:8-10,:21-26) is the
 * host libm's pow(c/255, 2.2).
 */

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
