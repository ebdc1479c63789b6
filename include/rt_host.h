/*
 * rt_host.h — C entry points of the host library (librt_host.so): the reference's scene builders, BVH build,
 * camera construction and output stage, exposed so that non-C++ callers (the Python test-suite and bench.py,
 * a Rust binding) can obtain an rt_scene_desc / rt_camera pair to hand to librt_amd (rt_amd.h).
 * Everything here is CPU-only host logic; no function in this header traces a ray.
 *
 * reference: scene functions src/main.rs:56-639, BVHNode::new src/bvh.rs:21-66 (called at src/main.rs:659),
 *            Camera::new src/camera.rs:54-110, color_to_rgb src/color.rs:12-19, PNG output src/renderer.rs:53-74.
 */
#ifndef RT_HOST_H
#define RT_HOST_H

#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_scene rth_scene; /* opaque: owns the object graph and its POD description */

typedef struct rth_scene_options {
    int32_t scene;             /* 0..8 as the reference's --scene (src/main.rs:47-49); other values -> 0 */
    int32_t bvh_policy;        /* 0 = reference (random-axis median split, src/bvh.rs:31-66), 1 = SAH   */
    uint64_t scene_seed;       /* seeds every build-time draw (object placement, Perlin tables, BVH axes) */
    int64_t image_width;       /* <= 0: the scene's in-code value                                        */
    double aspect_ratio;       /* <= 0: the scene's in-code value                                        */
    int32_t samples_per_pixel; /* <= 0: the scene's in-code value                                        */
    int32_t max_depth;         /* <= 0: the scene's in-code value                                        */
    const char *earth_image;   /* NULL: "synthetic:1024x512"; else a path (PPM, JPEG, PNG) or "synthetic:WxH"  */
} rth_scene_options;

/* Builds scene + top-level BVH + camera exactly as `main` does (src/main.rs:645-660) and describes them. */
int rth_scene_build(const rth_scene_options *options, rth_scene **out_scene);
void rth_scene_destroy(rth_scene *scene);
/* Borrowed pointers, valid until rth_scene_destroy. */
const rt_scene_desc *rth_scene_desc(const rth_scene *scene);
const rt_camera *rth_scene_camera(const rth_scene *scene);
/* Another view of the scene: Camera::new (src/camera.rs:54-110) over the CameraSettings the scene's builder used, with look_from and
 * look_at replaced (NULL: the scene's own).  With both NULL, *out is byte-identical to *rth_scene_camera(scene).  What
 * rt_render_views (rt_amd.h) takes one of per view. */
int rth_scene_camera_look(const rth_scene *scene, const double look_from[3] /* NULL: the scene's */,
                          const double look_at[3] /* NULL: the scene's */, rt_camera *out);
/* The scene's own look_from, look_at and vup (each may be NULL): what a caller turns to place other views (rtrace --orbit). */
int rth_scene_look(const rth_scene *scene, double look_from[3], double look_at[3], double vup[3]);
/* View k of an n-view orbit (rtrace --orbit n): the scene's look_from turned about the axis through look_at along vup by 360 k / n
 * degrees, counter-clockwise seen from vup's tip; k = 0 is look_from itself.  n >= 1. */
int rth_scene_orbit_look_from(const rth_scene *scene, int32_t k, int32_t n, double out_look_from[3]);

/* color_to_rgb(sum / spp) over a frame of per-pixel sums (src/renderer.rs:55-58, src/color.rs:12-19). */
int rth_resolve_rgb8(int32_t width, int32_t height, int32_t spp, const double *rgb_sum, uint8_t *out_rgb8);
/* The host mirrors of rt_tonemap_device and rt_log_average_luminance_device (rt_amd.h "tone mapping") on host memory: the same shared
 * per-value functions and the same reduction tree, so the bytes and the four doubles are the device's, bit for bit.  `values` holds
 * 3 * w * h doubles (sums with spp or the map spp_map, or means with spp = 1); out_rgb8 (3 * w * h bytes) and out_rgba8 (4 * w * h bytes,
 * alpha 0xff) may each be NULL, not both; out4 receives log_mean, Lavg, (double)count and 0.  They refuse what the device calls refuse
 * of these arguments, in the same order (-1, the field named in rth_last_error); there is no workspace and no stream. */
int rth_tonemap(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map /* NULL: uniform */,
                const rt_tonemap_params *params /* NULL: defaults */, uint8_t *out_rgb8, uint8_t *out_rgba8);
int rth_log_average_luminance(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map /* NULL: uniform */,
                              double delta, double *out4);
/* The host mirror of rt_film_device (rt_amd.h "film output") on host memory: the same shared encoders behind the same value, auto-exposure
 * through rth_log_average_luminance's tree, so `out` (rt_film_bytes(w, h, format) bytes, any alignment) holds the device's bytes, bit for
 * bit.  `values` as rth_tonemap takes them.  It refuses what the device call refuses of these arguments, in the same order and with the
 * same words (-1, the field named in rth_last_error); there is no workspace and no stream. */
int rth_film(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map /* NULL: uniform */,
             const rt_tonemap_params *tone /* NULL: defaults */, int32_t format /* RT_FILM_* */, void *out);
/* The host mirror of rt_bloom_device (rt_amd.h "bloom") on host memory: the same shared per-value functions in the same order, so
 * out_mean (3 * w * h doubles, a frame of means) holds the device's bits.  `values` as rth_tonemap takes them.  It refuses what the
 * device call refuses of these arguments, in the same order and with the same words (-1, the field named in rth_last_error); there is
 * no workspace and no stream. */
int rth_bloom(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map /* NULL: uniform */,
              const rt_bloom_params *params /* NULL: defaults */, double *out_mean);
/* The host mirror of rt_upsample_device (rt_amd.h "guided upsampling") on host memory: the same shared per-pixel functions in the same
 * order, so out_mean (3 * w * h doubles) and out_rgba8 (4 * w * h bytes, or NULL) hold the device's bits.  width and height are the FULL
 * size; `low` holds 3 * lw * lh doubles.  It refuses what the device call refuses of these arguments, in the same order and with the
 * same words (-1, the field named in rth_last_error); there is no workspace and no stream. */
int rth_upsample(int32_t width, int32_t height, const double *low, int32_t spp, const double *albedo_sum /* 3*w*h, or NULL */, int32_t albedo_spp,
                 const double *edge_sum /* 3*w*h, or NULL */, int32_t edge_spp, const rt_upsample_params *params /* NULL: defaults */,
                 double *out_mean, uint8_t *out_rgba8 /* or NULL */);
/* The host mirror of rt_robust_device (rt_amd.h "robust frames") on host memory: the same per-value body (csrc/rt_robust_shared.h), so
 * out_mean and, if it is not NULL, out_m2 (3 * w * h doubles each) hold the device's bits.  `stack` is blocks x 3 * w * h doubles, block
 * after block.  It refuses what the device call refuses, in the same order and with the same words (-1, the field named in
 * rth_last_error); there is no stream. */
int rth_robust(int32_t width, int32_t height, int32_t blocks, const double *stack, int32_t spp, const rt_robust_params *params /* NULL: defaults */,
               double *out_mean, double *out_m2 /* or NULL */);
/* The host mirror of rt_panorama_device (rt_amd.h "panoramas") on host memory: the same per-pixel body over the same tables
 * (rt_panorama_tables' 2 w + 2 h doubles) and the six faces (3 * F * F doubles each, face-major: sums with the count spp, or means with
 * spp = 1), so out_mean (3 * w * h doubles, a frame of means) holds the device's bits.  It refuses what the device call refuses, in the
 * same order and with the same words (-1, the field named in rth_last_error); there is no stream. */
int rth_panorama(int32_t width, int32_t height, const double *tables, const double *faces, int32_t face_size, int32_t guard, int32_t spp,
                 double *out_mean);
/* The host mirrors of rt_frame_error_device and rt_frame_noise_device (rt_amd.h "frame metrics") on host memory: the same shared pixel
 * term, combine and final values through the same reduction tree, so out8 (count, mse, rmse, rel_mse, mae, bias, max_abs, psnr) and
 * out4 (count, mean_var, noise, max_noise) hold the device's bits.  They refuse what the device calls refuse of these arguments, in the
 * same order and with the same words (-1, the field named in rth_last_error); there is no workspace and no stream. */
int rth_frame_error(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map /* NULL: uniform */,
                    const double *ref, int32_t ref_spp, const rt_frame_error_params *params /* NULL: defaults */, double *out8);
int rth_frame_noise(int32_t width, int32_t height, int32_t form /* RT_METRICS_* */, const double *a, const double *b, int32_t n,
                    const int32_t *spp_map /* NULL: uniform; sums form only */, const rt_frame_noise_params *params /* NULL: defaults */,
                    double *out4);
/* rth_write_pfm's counterpart: a colour PFM ("PF", either byte order by the scale's sign, the bottom row first) as 3 * w * h doubles,
 * row 0 on top, each the file's f32 widened; the scale's magnitude is not applied.  out_rgb may be NULL to query the size; `capacity`
 * is its room in doubles.  Every header number is bounded before it is multiplied: -1 (the reason in rth_last_error) for a width or
 * height < 1, w * h >= 2^27, a scale that is zero, not finite or not a number, trailing characters in a header field, or a body shorter
 * than the header announces.  Nothing beyond the file's bytes is read. */
int rth_read_pfm(const char *path, int32_t *out_width, int32_t *out_height, double *out_rgb, int64_t capacity);
/* RGB8 PNG writer (src/renderer.rs:59-72). */
int rth_write_png(const char *path, int32_t width, int32_t height, const uint8_t *rgb8);
/* The film formats' files, each from a frame in its format (rt_amd.h "film output"), row 0 on top:
 *   rth_write_hdr    RT_FILM_RGBE bytes as a Radiance picture: "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y h +X w\n", then the scanlines in
 *                    the new-style run-length code where 8 <= w <= 32767 (2 2 hi lo, then the four byte planes: a run is 128 + length and
 *                    the value, a literal its length, at most 128, and the bytes), as flat pixels otherwise;
 *   rth_write_pfm    RT_FILM_F32 floats as "PF\nw h\n-1.0\n", little-endian, the bottom row first;
 *   rth_write_png16  RT_FILM_RGB16 samples as a PNG of colour type 2 and bit depth 16 (big-endian in the file), through the filter and
 *                    zlib path of rth_write_png. */
int rth_write_hdr(const char *path, int32_t width, int32_t height, const uint8_t *rgbe);
int rth_write_pfm(const char *path, int32_t width, int32_t height, const float *rgb_f32);
int rth_write_png16(const char *path, int32_t width, int32_t height, const uint16_t *rgb16);
/* Deterministic procedural RGB8 map used where assets/earth-large.jpg is unavailable. */
int rth_synthetic_earth(int32_t width, int32_t height, uint8_t *out_rgb8);
/* Image ingest used by ImageTexture (PPM / JPEG, sequential or progressive / PNG / synthetic:WxH); out_rgb8 may be NULL to query size. */
int rth_load_image(const char *path, int32_t *out_width, int32_t *out_height, uint8_t *out_rgb8, int64_t capacity);

const char *rth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HOST_H */
