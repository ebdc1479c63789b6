// render(): the batch entry point.  reference: src/renderer.rs:12-75
// Same contract as the reference's `render(camera, world, output_file_name)`: trace every pixel, then
// divide by spp, gamma-encode, quantise and write `<output_file_name>.png` — but the pixel loop
// (src/renderer.rs:26-49) is one call into librt_amd (include/rt_amd.h) instead of a rayon par_iter.
// live_render(): the reference's second entry point (src/renderer.rs:77-137) without its window: the running-mean frame it refines
// one pass at a time, handed to a callback as the RGBA8 bytes the reference blits (include/rt_amd.h "live refinement").
#pragma once
#include "camera.hpp"
#include "hittable.hpp"
#include <functional>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace rt {

// The file render() writes (RenderOptions::format): the reference's 8-bit PNG, or one of the film formats of include/rt_amd.h "film output".
enum FilmFile { FILM_PNG = 0, FILM_PNG16 = 1, FILM_HDR = 2, FILM_PFM = 3 };

struct RenderOptions {
    uint64_t seed = 1; // render seed (the reference's RNG is unseeded; see include/rt_amd.h "RNG")
    int gpus = 1;      // framebuffer tiles are dealt round-robin to this many devices
    bool quiet = false;
    // > 0: render in passes of this many samples per pixel and rewrite the PNG after every pass.  It continues the SUM, so the
    // final image is bit-identical to a single-pass render (ranges accumulate exactly); the reference's running mean is live_render, below.
    int progressive_spp = 0;
    // live_render: samples per pixel folded into the running mean between two displayed frames (the reference: 1)
    int live_spp = 1;
    // adaptive sampling (include/rt_amd.h rt_render_adaptive) with these thresholds; the camera's spp is the maximum.  One GPU, single pass.
    bool adaptive = false;
    double adaptive_rel = 0.02;
    double adaptive_abs = 1e-3;
    int min_spp = 16, batch_spp = 16;
    // > 0: this many views in ONE rt_render_views call (include/rt_amd.h): view k looks from the camera's look_from turned about the
    // axis through look_at along vup by 360 k / orbit degrees (camera.hpp orbit_look_from), with seed + k, and goes to
    // <output_file_name>_<k as three digits>.png.  One GPU, single pass.
    int orbit = 0;
    // with `orbit`: the views go through rt_render_views_moments_device and are filtered as one stack by rt_denoise_views_device
    // (include/rt_amd.h "views denoise") with denoise_iters / denoise_sigma; each PNG is written from its view's filtered mean.
    bool orbit_denoise = false;
    // with `orbit`: the albedo-guided filter over the stack instead (rt_denoise_albedo_views_device, denoise_albedo_sigma).  The albedo
    // frames come from ONE rt_render_views_device over the albedo scene, under the views' cameras with background (1, 1, 1) and their
    // seeds, over the same sample range.
    bool orbit_denoise_albedo = false;
    // with `orbit`: an edge guide for the stack's filter (rt_denoise_guided_views_device, denoise_edges_sigma), alone — the plain filter
    // with the edge stop — or beside orbit_denoise / orbit_denoise_albedo.  The guide frames are one rt_render_views_device call over
    // the surface-ID scene, under the views' cameras with a black background and their seeds.
    bool orbit_denoise_edges = false;
    // the variance-guided à-trous denoiser (include/rt_amd.h "denoise") over the frame before it is written: a plain render then
    // goes through rt_render_moments_device, an adaptive one hands over its sums, sums of squares and spp map.  One GPU, single pass.
    bool denoise = false;
    int denoise_iters = 4;
    double denoise_sigma = 4.0;
    // with `denoise`: the albedo-guided filter instead (include/rt_amd.h "albedo-guided denoise").  The route creates the albedo scene
    // from the same description, renders it with rt_render_device over the same seed and sample range (an adaptive render: up to the
    // camera's spp) under the camera with background (1, 1, 1), and hands that frame to rt_denoise_albedo_device.
    bool denoise_albedo = false;
    double denoise_albedo_sigma = 0.5;
    // with `denoise`: an edge guide for the filter (include/rt_amd.h "edge-guided denoise"), alone or beside `denoise_albedo`.  The
    // route creates the surface-ID scene from the same description, renders it with rt_render_device over the same seed and sample
    // range (an adaptive render: up to the camera's spp) under the camera with background (0, 0, 0), and hands that frame to
    // rt_denoise_guided_device as d_edge_sum; denoise_edges_sigma is the filter's sigma_edge.
    bool denoise_edges = false;
    double denoise_edges_sigma = 0.5;
    // live_render: every displayed frame goes through the filter (include/rt_amd.h "live denoise").  A pass is then
    // rt_render_mean_moments_device — the running mean with Welford's M2 beside it — and rt_denoise_mean_device with denoise_iters /
    // denoise_sigma into a separate display frame: the running mean and M2 are never overwritten by the filter.
    bool live_denoise = false;
    // with `live_denoise`: the albedo-guided filter (rt_denoise_albedo_mean_device, denoise_albedo_sigma).  Each pass also folds the
    // albedo scene's samples of the same range, under the camera with background (1, 1, 1), into a running albedo mean
    // (rt_render_mean_device).
    bool live_denoise_albedo = false;
    // with `live_denoise`: > 0 sends every pass through rt_denoise_mean_spatial_device / rt_denoise_albedo_mean_spatial_device with
    // spatial_below = this (include/rt_amd.h "spatial variance"): frames of fewer samples take their variance from the spread of the
    // neighbouring pixels, so the first pass is shown filtered too.  0: off, the means forms as they are.
    int live_denoise_spatial = 0;
    // live_render: an edge guide for every displayed frame's filter (include/rt_amd.h "edge guide on every route"), alone or beside
    // live_denoise_albedo and live_denoise_spatial; it turns the filter on.  The surface-ID scene is rendered ONCE per session, before
    // the first pass, as a frame of means (rt_render_mean_device over min(spp - 1, 16) samples under the camera with a black background
    // and the session's seed), and every pass goes through rt_denoise_guided_mean_device or, with live_denoise_spatial,
    // rt_denoise_guided_mean_spatial_device; denoise_edges_sigma is the filter's sigma_edge.  Not with `upsample` (live_render throws).
    bool live_denoise_edges = false;
    int denoise_spatial_radius = 1; // its window_radius, 1..3
    // the tone-mapping stage (include/rt_amd.h "tone mapping") in the output stage's place, on every single-GPU route: the final bytes
    // come from rt_tonemap_device — a plain render's and an unfiltered orbit's from its host mirror rth_tonemap, the same bytes — on the
    // route's sums (adaptive: with the spp map), the filters' means, or the live route's running mean.  tonemap is the operator
    // (RT_TONEMAP_*); -1: the stage is off and every route is what it is without it.  Orbit handles each view as a frame of its own.
    int tonemap = -1;
    double exposure_ev = 0.0;       // stops: the stage's exposure is exp2(exposure_ev)
    double auto_exposure = 0.0;     // > 0: the key the frame's log-average luminance is mapped to (auto_key); 0: off
    double tonemap_white = std::numeric_limits<double>::infinity(); // Reinhard's white
    // bloom (include/rt_amd.h "bloom") in front of the tone-mapping stage, wherever that stage runs: the route's sums or means go through
    // rt_bloom_device — a plain render's and an unfiltered orbit's through its host mirror rth_bloom, the same bits — and the stage takes
    // the bloomed means with spp = 1, auto-exposure included.  bloom is the strength; < 0: off.  With bloom on and tonemap < 0 the
    // stage runs with the clamp.  Orbit blooms each view on its own.
    double bloom = -1.0;
    double bloom_threshold = 1.0;   // luminance above which a pixel glows
    int bloom_levels = 5;           // K, 1..8: a glow of radius 2 * (2^K - 1) pixels
    // guided upsampling (include/rt_amd.h "guided upsampling"): upsample = F in 2..4 traces the beauty frame under rt_camera_scaled —
    // 1 / F^2 of the paths — and brings it to the camera's size with rt_upsample_device; 0: off.  upsample_albedo / upsample_edges
    // render the full-size albedo / surface-ID frame (the denoise routes' guide scenes and cameras, the render's seed and spp) as the
    // upsampler's guides.  With `denoise` on, the filter — and its own guides — run at the low size, in front of the upsampler;
    // bloom and the tone-mapping stage run behind it on the full-size means.  One GPU, one pass; not on the adaptive, orbit or
    // progressive routes (render() throws).  live_render: every pass traces — and with live_denoise* filters — the small frame and
    // shows the upsampled one; the full-size guide frames are rendered once, before the first pass, at min(spp - 1, 16) samples per
    // pixel, and they, the full-size frame and the upsampler's workspace are kept across the passes.
    int upsample = 0;
    bool upsample_albedo = false;
    bool upsample_edges = false;
    // robust frames (include/rt_amd.h "robust frames"): robust_blocks = K in 1..32 renders K sub-frames of spp / K samples under the
    // camera with seeds seed + k in ONE rt_render_views_device call and combines them with rt_robust_device; 0: off.  K must divide the
    // camera's spp.  The PNG comes from the robust means through the means-form output (rt_resolve_rgba8_device, or bloom and the
    // tone-mapping stage); with `denoise` the combiner writes M2 as well and the frame goes through rt_denoise_mean_device with
    // samples = K.  One GPU, one pass; not with adaptive, orbit, progressive_spp, upsample, the guided filters or live_render (they throw).
    int robust_blocks = 0;
    int robust_mode = RT_ROBUST_GINI;   // RT_ROBUST_*
    int robust_trim = 1;                // RT_ROBUST_TRIM's count
    double robust_gain = 0.0;           // RT_ROBUST_GINI's gain; <= 0: the library's default
    // film output (include/rt_amd.h "film output"): FILM_PNG16, FILM_HDR or FILM_PFM sends the frame of every single-GPU, one-pass route
    // — plain, adaptive, the denoise family, robust, upsample, each view of orbit and live_render's final frame — through the film stage
    // (rt_film_device; a plain render's and an unfiltered orbit's through its host mirror rth_film, the same bytes) in the tone-mapping
    // stage's place, behind bloom, with that stage's operator, exposure and key, and writes NAME.png (16-bit), NAME.hdr or NAME.pfm.  With
    // no tonemap, exposure or bloom given the stage runs with the clamp and exposure 1: .hdr and .pfm hold the linear means.  Not with
    // gpus > 1 or progressive_spp (render() throws).
    int format = FILM_PNG;
    // panoramas (include/rt_amd.h "panoramas"): panorama_width = W > 0 (even) renders the six cube-face views about panorama_at (or, not
    // given, the camera's centre) — panorama_face pixels wide (0: W / 4 + 2 * panorama_guard) with panorama_guard guard texels, under seeds
    // seed + face — in ONE rt_render_views_device call and resamples them with rt_panorama_device into a W x W / 2 equirectangular frame of
    // means, which goes through bloom, the tone-mapping stage and the film formats as any frame of means.  The scene camera's image size is
    // not used.  Not with adaptive, orbit, progressive_spp, upsample, robust_blocks, denoise or gpus > 1 (render() throws), nor live_render.
    int panorama_width = 0;
    int panorama_face = 0;
    int panorama_guard = 1;
    bool panorama_at_given = false;
    double panorama_at[3] = {0.0, 0.0, 0.0};
    // frame metrics (include/rt_amd.h "frame metrics"): compare_file names a colour PFM of the frame's size, a frame of means.  On every
    // single-GPU, one-pass route that ends in one frame of sums or means — plain, adaptive, the denoise family, upsample, robust,
    // panorama — render() measures the values the output stage is about to read (behind the filter, the combiner, the upsampler or the
    // resampler; in front of bloom and the tone mapping) against it with rt_frame_error_device (a plain render, whose sums are on the
    // host: its mirror rth_frame_error, the same bits) and prints one line,
    //     metrics: count=… mse=… rmse=… relmse=… mae=… bias=… max=… psnr=…        (every double as %.17g)
    // compare_eps is the call's eps; <= 0: the library's default.  It throws on a file the reader refuses and on a size mismatch.  Not
    // with orbit, progressive_spp or gpus > 1 (render() throws), nor live_render (it throws).
    std::string compare_file;
    double compare_eps = 0.0;
    // live_render: live_stop_noise >= 0 evaluates rt_frame_noise_device (means form) on the running mean and M2 after every pass and ends
    // the loop at the first pass with samples >= live_stop_min_samples and noise <= live_stop_noise (or, as without it, at spp - 1
    // samples).  The loop takes the moments route if it is not on it already (rt_render_mean_moments_device writes the same mean and
    // bytes), so the frames shown before the stop are those of the same run without it.  Where the pass itself writes the display bytes,
    // the four doubles lie behind them in one buffer and come back in the frame's own download; one line per pass (unless quiet),
    //     live-stop-pass: samples=… noise=…
    // and a final  live-stop: samples=… noise=…  (%.17g) are printed.  < 0: off.
    double live_stop_noise = -1.0;
    int live_stop_min_samples = 16;
};

// rt_frame_error_device on device 0 over DEVICE frames: d_values (sums with spp or, if d_spp is not null, a device map; means with
// spp = 1) against d_ref (sums with ref_spp; means with 1); eps <= 0: the library's default.  Allocates the workspace and the output,
// waits, and writes count, mse, rmse, rel_mse, mae, bias, max_abs, psnr to out8.  frame_noise_device: rt_frame_noise_device likewise
// (form RT_METRICS_*; d_a, d_b the moments, n their count) into out4: count, mean_var, noise, max_noise.  Both throw std::runtime_error
// on a library error.
void frame_error_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const double *d_ref, int32_t ref_spp,
                        double eps, double out8[8]);
void frame_noise_device(int32_t width, int32_t height, int32_t form, const double *d_a, const double *d_b, int32_t n, const int32_t *d_spp, double eps,
                        double out4[4]);

// rt_denoise_device on device 0 over DEVICE frames of sums and sums of squares (3 * w * h doubles each) with the uniform sample count
// `spp` or, if d_spp is not null, a device map of w * h int32: allocates the workspace and the outputs, runs the filter with
// opt.denoise_iters / opt.denoise_sigma and returns the display frame's RGB bytes (3 * w * h).  Throws std::runtime_error on a GPU
// library error.
std::vector<uint8_t> denoise(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                             const RenderOptions &opt = {});

// rt_denoise_albedo_device likewise: d_albedo_sum is a DEVICE frame of 3 * w * h doubles, the sums of albedo_spp samples of the albedo
// scene; opt.denoise_albedo_sigma is the filter's sigma_albedo.
std::vector<uint8_t> denoise_albedo(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                                    const double *d_albedo_sum, int32_t albedo_spp, const RenderOptions &opt = {});

// rt_denoise_guided_device likewise: d_edge_sum is a DEVICE frame of 3 * w * h doubles, the sums of edge_spp samples of the edge guide
// (the surface-ID scene's render); d_albedo_sum may be null (no albedo guide: albedo_spp is not read); opt.denoise_edges_sigma is the
// filter's sigma_edge.
std::vector<uint8_t> denoise_guided(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                                    const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp,
                                    const RenderOptions &opt = {});

// rt_denoise_views_device and rt_denoise_albedo_views_device likewise, over a stack of n_views frames, view-major in every DEVICE
// buffer, with the uniform sample count `spp`: the RGB bytes of the n_views display frames, one behind the other (n_views * 3 * w * h).
std::vector<uint8_t> denoise_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const RenderOptions &opt = {});
std::vector<uint8_t> denoise_albedo_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                          const double *d_albedo_sum, int32_t albedo_spp, const RenderOptions &opt = {});

// rt_denoise_mean_device and rt_denoise_albedo_mean_device likewise, over DEVICE frames of running means and of M2 after `samples`
// samples of every pixel (rt_render_mean_moments_device) and, guided, the albedo scene's running mean (rt_render_mean_device).
std::vector<uint8_t> denoise_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                  const RenderOptions &opt = {});
std::vector<uint8_t> denoise_albedo_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                         const double *d_albedo_mean, const RenderOptions &opt = {});

// rt_denoise_guided_mean_device likewise — with opt.live_denoise_spatial > 0, rt_denoise_guided_mean_spatial_device and its params as
// below —: d_edge_mean is a DEVICE frame of 3 * w * h doubles, the means of the edge guide; d_albedo_mean may be null (no albedo guide).
std::vector<uint8_t> denoise_guided_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                         const double *d_albedo_mean, const double *d_edge_mean, const RenderOptions &opt);
// rt_denoise_guided_views_device likewise, over a stack of n_views frames, view-major in every DEVICE buffer; d_albedo_sum may be null.
std::vector<uint8_t> denoise_guided_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                          const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp,
                                          const RenderOptions &opt);
// rt_denoise_mean_spatial_device and rt_denoise_albedo_mean_spatial_device likewise, with spatial_below = opt.live_denoise_spatial (0:
// the library's default) and window_radius = opt.denoise_spatial_radius; d_m2 may be null where samples < spatial_below.
std::vector<uint8_t> denoise_mean_spatial(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                          const RenderOptions &opt = {});
std::vector<uint8_t> denoise_albedo_mean_spatial(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                                 const double *d_albedo_mean, const RenderOptions &opt = {});

// The tone-mapping stage with opt's operator, exposure, key and white.  tonemap_rgb8: on a HOST frame of sums (3 * w * h doubles) with
// the uniform count spp, through the host mirror; returns 3 * w * h bytes.  tonemap_device: rt_tonemap_device on device 0 over a
// DEVICE frame (sums with spp or, if d_spp is not null, a device map; means with spp = 1); returns 3 * w * h bytes, or with `rgba`
// 4 * w * h.  Both throw std::runtime_error on a library error.
std::vector<uint8_t> tonemap_rgb8(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt);
std::vector<uint8_t> tonemap_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, bool rgba,
                                    const RenderOptions &opt);

// The film stage likewise, in the format of opt.format's file (FILM_HDR: RT_FILM_RGBE, FILM_PFM: RT_FILM_F32, FILM_PNG16: RT_FILM_RGB16):
// film_host through the host mirror rth_film on a HOST frame, film_device through rt_film_device on device 0 over a DEVICE frame; both
// return rt_film_bytes(w, h, format) bytes.  write_film_frame writes such a frame to NAME.hdr / NAME.pfm / NAME.png.
std::vector<uint8_t> film_host(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt);
std::vector<uint8_t> film_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const RenderOptions &opt);
void write_film_frame(const std::string &name, int32_t width, int32_t height, const std::vector<uint8_t> &film, const RenderOptions &opt);

// rt_panorama_device on device 0: the six DEVICE frames of 3 * F * F doubles at d_faces (sums with the count spp, or means with spp = 1),
// F = face_size with `guard` guard texels, into the DEVICE frame d_mean_out (3 * width * height doubles of means).  The tables of the
// size are made and uploaded by the call and freed behind it.  Throws std::runtime_error on a library error.
void panorama_device(int32_t width, int32_t height, const double *d_faces, int32_t face_size, int32_t guard, int32_t spp, double *d_mean_out);

// Bloom with opt's strength, threshold and levels.  bloom_means: on a HOST frame (sums with the uniform count spp; means with spp = 1),
// through the host mirror; returns the 3 * w * h bloomed means.  bloom_device: rt_bloom_device on device 0 over a DEVICE frame (sums with
// spp or, if d_spp is not null, a device map; means with spp = 1) into the DEVICE frame d_mean_out (3 * w * h doubles, not d_values):
// the frame stays on the device; the call's workspace is allocated and freed here, and it returns when the frame is written.  Both throw
// std::runtime_error on a library error.
std::vector<double> bloom_means(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt);
void bloom_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, double *d_mean_out, const RenderOptions &opt);

// rt_robust_device on device 0 with opt's mode, trim and gain: `blocks` DEVICE frames of 3 * w * h doubles at d_stack, block after
// block (sums with the per-block count spp; means with spp = 1), into the DEVICE frames d_mean_out and, if not null, d_m2_out.  Enqueued
// on the null stream, not waited for.  Throws std::runtime_error on a library error.
void robust_device(int32_t width, int32_t height, int32_t blocks, const double *d_stack, int32_t spp, double *d_mean_out, double *d_m2_out,
                   const RenderOptions &opt);

// Guided upsampling with opt's factor and the library's default stops; width x height is the FULL size, the low frame holds
// 3 * ceil(w / F) * ceil(h / F) values (sums with the count spp; means with spp = 1), each guide 3 * w * h sums with its count, or null /
// empty.  upsample_means: on HOST frames, through the host mirror rth_upsample; returns the 3 * w * h full-size means.
// upsample_device: rt_upsample_device on device 0 over DEVICE frames into the DEVICE frame d_mean_out: the frame stays on the device;
// the call's workspace is allocated and freed here, and it returns when the frame is written.  Both throw std::runtime_error on a
// library error.
std::vector<double> upsample_means(const std::vector<double> &low, int32_t width, int32_t height, int32_t spp, const std::vector<double> &albedo_sum,
                                   int32_t albedo_spp, const std::vector<double> &edge_sum, int32_t edge_spp, const RenderOptions &opt);
void upsample_device(int32_t width, int32_t height, const double *d_low, int32_t spp, const double *d_albedo_sum, int32_t albedo_spp,
                     const double *d_edge_sum, int32_t edge_spp, double *d_mean_out, const RenderOptions &opt);

// Returns the per-pixel sums (w*h*3 doubles, row-major) exactly like the reference's `raw_pixels`
// (src/renderer.rs:26-49).  Throws std::runtime_error if the GPU library reports an error.
// `on_pass(sums, samples_done)`, if given, is called after every progressive pass.
std::vector<double> render_sums(const Camera &camera, const Hittable &world, const RenderOptions &opt = {},
                                const std::function<void(const std::vector<double> &, int)> &on_pass = nullptr);

// color_to_rgb(c / spp) over the whole frame (src/renderer.rs:55-58)
std::vector<uint8_t> resolve_rgb8(const std::vector<double> &sums, int32_t spp);

// The reference's live_render (src/renderer.rs:77-137) without the window, on device 0: passes of opt.live_spp samples per pixel are
// folded into a running mean, avg += (new - avg) / num_samples (:114), and after every pass on_frame(rgba8, num_samples) gets the
// frame the reference would show — color_to_rgb(avg) with alpha 0xff, 4 * w * h bytes (:124-126) — and the number of samples in it.
// It ends as the reference's loop does: that loop starts at num_samples = 1 and draws only `if num_samples < spp` (:104), so its
// divisors are 1 .. spp - 1 and the frame it settles on holds spp - 1 samples, not spp.  Returns the last frame (all (0, 0, 0, 0xff),
// the reference's zeroed raw_pixels, when spp <= 1 leaves nothing to draw).  Throws std::runtime_error on a GPU library error.
// With opt.live_denoise the frame handed over is the filtered one (above); the loop still settles on spp - 1 samples.  With
// opt.live_denoise_spatial as well, that holds from the first pass on.
// The frames shown are RGBA8 whatever opt.format says; with a film format and final_film not null, *final_film receives the last
// frame in that format (bloom and the film stage over the means the last frame shown was made from).
std::vector<uint8_t> live_render(const Camera &camera, const Hittable &world, const RenderOptions &opt = {},
                                 const std::function<void(const std::vector<uint8_t> &, int)> &on_frame = nullptr,
                                 std::vector<uint8_t> *final_film = nullptr);

void render(std::shared_ptr<Camera> camera, std::shared_ptr<Hittable> world, const std::string &output_file_name,
            const RenderOptions &opt = {});

} // namespace rt
