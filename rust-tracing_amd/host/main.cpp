// Command-line front end.  reference: src/main.rs:40-54 (Args) and :641-669 (main)
//   -s/--scene N, -o/--output NAME, -l/--live as in the reference.  -l/--live [--live-spp K] refines the frame as the reference's
//   live_render does (running mean, K samples per pixel between two frames, spp - 1 samples in all: renderer.hpp) and, there being no
//   window, writes the last frame's RGB bytes to OUTPUT.png; the reference's live mode writes no file, so -o must name one.
//   Added: --width/--aspect/--spp/--depth (BASELINE.json's configs change these),
//   --seed/--scene-seed, --gpus, --earth PATH|synthetic:WxH, --bvh reference|sah, --progressive N (rewrite the PNG
//   every N samples per pixel; continues the sum, not the running mean), --adaptive REL
//   [--adaptive-abs A] [--min-spp N] [--batch-spp N] (per-pixel sample counts from a variance bound; --spp is the maximum),
//   --denoise [--denoise-iters K] [--denoise-sigma X] (the variance-guided à-trous filter of include/rt_amd.h over the frame before
//   it is written; with --adaptive it takes the adaptive sums and the spp map),
//   --denoise-albedo [--denoise-albedo-sigma X] (implies --denoise: the albedo-guided filter, with a first-hit albedo frame rendered
//   from the scene's albedo scene over the same seed and samples),
//   --denoise-edges [--denoise-edges-sigma X] (implies --denoise, alone or with --denoise-albedo: the filter also stops at the edges of
//   a first-hit surface-ID frame rendered from the scene's surface-ID scene over the same seed and samples),
//   -l --live-denoise [--denoise-iters K] [--denoise-sigma X] (every live frame through the filter, from the running mean and Welford's
//   M2: include/rt_amd.h "live denoise"), --live-denoise-albedo [--denoise-albedo-sigma X] (implies --live-denoise: the guided filter,
//   with a running albedo mean folded over the same samples), --live-denoise-spatial [N] [--denoise-spatial-radius R] (with
//   --live-denoise[-albedo]: frames of fewer than N samples, default 2, take their variance from the spread of the neighbouring
//   pixels over a (2R + 1)^2 window, so the first frame is filtered too: include/rt_amd.h "spatial variance"),
//   --live-denoise-edges [--denoise-edges-sigma X] (implies --live-denoise, alone or with --live-denoise-albedo and
//   --live-denoise-spatial: every frame's filter also stops at the edges of a surface-ID frame rendered once per session, and the
//   spatial window keeps to its centre's surface: include/rt_amd.h "edge guide on every route"; not with --upsample),
//   --orbit N (N views around the scene's look_at in one launch: OUTPUT_000.png .. OUTPUT_<N-1>.png, view k with seed + k).
//   --orbit N --orbit-denoise [--denoise-iters K] [--denoise-sigma X] (the views' sums and sums of squares from one launch, filtered as
//   one stack: include/rt_amd.h "views denoise"), --orbit-denoise-albedo [--denoise-albedo-sigma X] (the guided filter instead, its albedo
//   frames from one views launch over the albedo scene), --orbit-denoise-edges [--denoise-edges-sigma X] (alone, or beside either of
//   the two: the stack's filter also stops at the edges of the views' surface-ID frames, rendered in one views launch).
//   --tonemap clamp|reinhard|aces, --exposure EV, --auto-exposure [KEY], --tonemap-white W (the tone-mapping stage of include/rt_amd.h
//   in the output stage's place, on every single-GPU route: the bytes of the PNG — each PNG of --orbit, each frame of --live — come
//   from the route's sums or means exposed by 2^EV, or by KEY over the frame's log-average luminance, through the operator).
//   --bloom [STRENGTH] [--bloom-threshold T] [--bloom-levels K] (bloom of include/rt_amd.h in front of that stage, wherever it runs: the
//   light of the pixels above luminance T is spread over K a-trous levels and added back STRENGTH times; alone it implies the stage with
//   the clamp).
//   --upsample F [--upsample-albedo] [--upsample-edges] (guided upsampling of include/rt_amd.h: the beauty frame is traced at 1/F of the
//   width and height, F = 2..4, and brought to full size under the full-size albedo and surface-ID frames asked for; the --denoise
//   and --live-denoise families then filter the small frame, and bloom and the tone mapping run on the full-size one; --live renders the
//   guide frames once per session).
//   --compare REF.pfm [--compare-eps E] (frame metrics of include/rt_amd.h: the frame the output stage is about to read, against a PFM of
//   its size; one line `metrics: ...`), -l --live-stop X [--live-stop-min N] (the live loop ends once the frame's noise is at most X),
//   --robust K [--robust-mode mean|trim|median|gini] [--robust-trim T] [--robust-gain X] (robust frames of include/rt_amd.h: K sub-frames
//   of spp / K samples under seeds seed + k in one views launch, combined by the median of means; --denoise filters the result with
//   samples = K, --bloom and --tonemap run behind it).
//   --panorama W [--panorama-face F] [--panorama-guard G] [--panorama-at x,y,z] (panoramas of include/rt_amd.h: the six cube-face views
//   about a point in one views launch, resampled on the device into a W x W / 2 equirectangular frame of means; --bloom, --tonemap and
//   --format run behind it).
//   --format png|png16|hdr|pfm (film output of include/rt_amd.h: the frame of every single-GPU, one-pass route — each file of --orbit,
//   the last frame of --live — as a 16-bit PNG, a Radiance OUTPUT.hdr or a float OUTPUT.pfm; --tonemap, --exposure, --auto-exposure,
//   --tonemap-white and --bloom apply in front of every format, and with none of them .hdr and .pfm hold the linear means).
#include "image_io.hpp"
#include "renderer.hpp"
#include "scenes.hpp"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

using namespace rt;

static void usage(const char *argv0) {
    fprintf(stderr,
            "Usage: %s [-s SCENE] [-o OUTPUT] [--width W] [--aspect A] [--spp N] [--depth D]\n"
            "          [--seed S] [--scene-seed S] [--gpus N] [--progressive SPP_PER_PASS] [--earth PATH|synthetic:WxH] [--bvh reference|sah]\n"
            "          [--adaptive REL [--adaptive-abs A] [--min-spp N] [--batch-spp N]]   (one GPU; --spp is the maximum)\n"
            "          [--denoise [--denoise-iters K] [--denoise-sigma X]]   (one GPU, one pass: the PNG is written from the denoised mean; K from 1 to 6,\n"
            "                         default 4; X > 0, default 4; also with --adaptive)\n"
            "          [--denoise-albedo [--denoise-albedo-sigma X]]   (implies --denoise: the filter is guided by a first-hit albedo frame as well and works on\n"
            "                         the frame divided by it; X > 0, default 0.5: the albedo difference at which a tap's weight is 0)\n"
            "          [--denoise-edges [--denoise-edges-sigma X]]   (implies --denoise, alone or with --denoise-albedo: the filter also stops where a first-hit\n"
            "                         surface-ID frame changes; X > 0, default 0.5: the difference of that frame at which a tap's weight is 0)\n"
            "          [-l|--live [--live-spp K] -o OUTPUT]   (one GPU: the reference's live mode without the window — a running mean refined K samples\n"
            "                         per pixel at a time, default 1, over spp - 1 samples; the last frame goes to OUTPUT.png)\n"
            "          [--live-denoise [--denoise-iters K] [--denoise-sigma X]]   (with -l/--live: every frame shown is the à-trous filter's, from the running\n"
            "                         mean and a running second moment; the mean itself is not touched)\n"
            "          [--live-denoise-albedo [--denoise-albedo-sigma X]]   (implies --live-denoise: the albedo-guided filter, with a running first-hit albedo\n"
            "                         mean over the same samples)\n"
            "          [--live-denoise-spatial [N] [--denoise-spatial-radius R]]   (with --live-denoise or --live-denoise-albedo: frames of fewer than N\n"
            "                         samples, default 2, take their variance from the neighbouring pixels' spread, so the first frame is filtered too;\n"
            "                         R from 1 to 3, default 1: the window is (2R + 1) x (2R + 1) pixels)\n"
            "          [--live-denoise-edges [--denoise-edges-sigma X]]   (implies --live-denoise, alone or with --live-denoise-albedo and\n"
            "                         --live-denoise-spatial: the filter also stops where a first-hit surface-ID frame, rendered once per session,\n"
            "                         changes, and the spatial window keeps to its centre's surface; not with --upsample)\n"
            "          [--orbit N]   (N from 1 to 1000, the file names' three digits; one GPU, one launch: N views, look_from turned about the axis through look_at along vup by\n"
            "                         360 k / N degrees, view k with seed + k, written to OUTPUT_000.png .. OUTPUT_<N-1>.png)\n"
            "          [--orbit-denoise [--denoise-iters K] [--denoise-sigma X]]   (with --orbit: every view through the à-trous filter, all views in\n"
            "                         one set of launches, from sums and sums of squares rendered in one launch)\n"
            "          [--orbit-denoise-albedo [--denoise-albedo-sigma X]]   (with --orbit, instead of --orbit-denoise: the albedo-guided filter, with\n"
            "                         first-hit albedo frames of the same views rendered in one launch)\n"
            "          [--orbit-denoise-edges [--denoise-edges-sigma X]]   (with --orbit, alone or beside --orbit-denoise or --orbit-denoise-albedo:\n"
            "                         the views' filter also stops where their first-hit surface-ID frames, rendered in one launch, change)\n"
            "          [--tonemap clamp|reinhard|aces] [--exposure EV] [--auto-exposure [KEY]] [--tonemap-white W]   (one GPU, any route but --progressive:\n"
            "                         the final bytes go through an exposure and a tone curve before the gamma; EV in stops, |EV| <= 64, default 0;\n"
            "                         KEY > 0, default 0.18: the exposure maps the frame's log-average luminance to KEY; W > 0: with --tonemap reinhard,\n"
            "                         the value that maps to white, default none; --orbit exposes each view on its own)\n"
            "          [--bloom [STRENGTH] [--bloom-threshold T] [--bloom-levels K]]   (one GPU, any route but --progressive: in front of the tone\n"
            "                         mapping, the light of the pixels whose luminance is above T, default 1, is blurred over K = 1..8 levels,\n"
            "                         default 5 (a glow of radius 2 * (2^K - 1) pixels), and added back STRENGTH >= 0 times, default 0.25; alone it\n"
            "                         implies --tonemap clamp; --orbit blooms each view on its own)\n"
            "          [--compare REF.pfm [--compare-eps E]]   (one GPU, one pass; not with -l, --orbit or --progressive: the frame's means, behind\n"
            "                         the filters and in front of bloom and the tone mapping, against the PFM of the same size; prints one line\n"
            "                         metrics: count= mse= rmse= relmse= mae= bias= max= psnr=)\n"
            "          [--live-stop X [--live-stop-min N]]   (with -l/--live: the noise of the running mean, the RMS relative standard error of the\n"
            "                         pixel means, after every pass; the loop ends at the first pass with at least N samples, default 16, whose\n"
            "                         noise is at most X, and prints live-stop: samples= noise=)\n"
            "          [--upsample F [--upsample-albedo] [--upsample-edges]]   (one GPU; a plain render, the --denoise family or --live: the frame is\n"
            "                         traced at 1/F of the width and height, F = 2, 3 or 4 — 1/F^2 of the paths — and brought to full size by a\n"
            "                         joint bilateral upsampler; --upsample-albedo multiplies the full-size first-hit albedo frame back in,\n"
            "                         --upsample-edges stops the interpolation at the edges of the full-size surface-ID frame; --denoise* and\n"
            "                         --live-denoise* then filter the small frame, and --live renders the guides once, at up to 16 spp; not with\n"
            "                         --orbit, --adaptive, --gpus > 1 or --progressive)\n"
            "          [--robust K [--robust-mode mean|trim|median|gini] [--robust-trim T] [--robust-gain X]]   (one GPU, one launch: K = 1..32 sub-frames\n"
            "                         of spp / K samples each — K must divide spp — under seeds seed + k, combined per value by the median of means:\n"
            "                         a trimmed mean of the K block means that drops T at each end (trim), all but the centre (median), none (mean),\n"
            "                         or, default, as many as X times the blocks' Gini coefficient asks for (gini; X > 0, default 1); fireflies stay\n"
            "                         in their block and are trimmed; --denoise then filters the robust frame with samples = K; also with --tonemap\n"
            "                         and --bloom; not with -l, --adaptive, --orbit, --progressive, --upsample, --gpus > 1, --denoise-albedo, --denoise-edges)\n"
            "          [--format png|png16|hdr|pfm]   (one GPU, any route but --progressive: the file written — each file of --orbit, the last frame\n"
            "                         of --live — is OUTPUT.png with 8-bit samples, default, or 16-bit ones (png16), a Radiance OUTPUT.hdr with shared-\n"
            "                         exponent pixels (hdr) or a float OUTPUT.pfm (pfm); --tonemap, --exposure, --auto-exposure, --tonemap-white and\n"
            "                         --bloom apply in front of every format: with none of them hdr and pfm hold the linear means, unclipped)\n"
            "          [--panorama W [--panorama-face F] [--panorama-guard G] [--panorama-at x,y,z]]   (one GPU, one launch: a 360 x 180 degree\n"
            "                         equirectangular frame of W x W / 2 pixels, W even, seen from x,y,z (default: the scene camera's centre): the six\n"
            "                         faces of a cube map, F pixels wide (default W / 4 + 2 G) with G guard texels beyond the 90 degrees (default 1),\n"
            "                         under seeds seed + face, resampled bilinearly; the frame of means goes on through --bloom, --tonemap, --exposure,\n"
            "                         --auto-exposure and --format as any other: --format hdr is what viewers and image-based lighting read; not with\n"
            "                         -l, --adaptive, --orbit, --progressive, --upsample, --robust, --gpus > 1 or the --denoise family)\n"
            "  scenes: 0 random balls, 1 two spheres, 2 earth, 3 perlin spheres, 4 quads, 5 simple light,\n"
            "          6 cornell box, 7 cornell smoke, 8 final scene\n",
            argv0);
}

int main(int argc, char **argv) {
    int scene = 0;
    bool live = false, output_given = false, live_spp_given = false, denoise_knob_given = false, albedo_knob_given = false, spatial_knob_given = false, edges_knob_given = false, tonemap_given = false, white_given = false, bloom_knob_given = false, robust_knob_given = false, panorama_knob_given = false, compare_eps_given = false, live_stop_min_given = false;
    std::string output = "output";
    SceneOptions so;
    so.earth_image = "assets/earth-large.jpg"; // the reference's default (src/main.rs:179,:591); --earth synthetic:WxH needs no file
    RenderOptions ro;
    uint64_t scene_seed = 1;

    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char *name) -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", name); usage(argv[0]); exit(2); }
            return argv[++i];
        };
        if (a == "-l" || a == "--live") live = true;
        else if (a == "-s" || a == "--scene") scene = atoi(need("--scene"));
        else if (a == "-o" || a == "--output") { output = need("--output"); output_given = true; }
        else if (a == "--width") so.image_width = atoll(need("--width"));
        else if (a == "--aspect") so.aspect_ratio = atof(need("--aspect"));
        else if (a == "--spp") so.samples_per_pixel = atoi(need("--spp"));
        else if (a == "--depth") so.max_depth = atoi(need("--depth"));
        else if (a == "--seed") ro.seed = strtoull(need("--seed"), nullptr, 10);
        else if (a == "--scene-seed") scene_seed = strtoull(need("--scene-seed"), nullptr, 10);
        else if (a == "--gpus") ro.gpus = atoi(need("--gpus"));
        else if (a == "--progressive") ro.progressive_spp = atoi(need("--progressive"));
        else if (a == "--live-spp") {
            ro.live_spp = atoi(need("--live-spp")); live_spp_given = true;
            if (ro.live_spp < 1) { fprintf(stderr, "--live-spp needs a number of samples per frame of at least 1\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--adaptive") { ro.adaptive = true; ro.adaptive_rel = atof(need("--adaptive")); }
        else if (a == "--adaptive-abs") ro.adaptive_abs = atof(need("--adaptive-abs"));
        else if (a == "--min-spp") ro.min_spp = atoi(need("--min-spp"));
        else if (a == "--batch-spp") ro.batch_spp = atoi(need("--batch-spp"));
        else if (a == "--denoise") ro.denoise = true;
        else if (a == "--denoise-iters") {
            ro.denoise_iters = atoi(need("--denoise-iters")); denoise_knob_given = true;
            if (ro.denoise_iters < 1 || ro.denoise_iters > 6) { fprintf(stderr, "--denoise-iters needs a number of iterations from 1 to 6\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--denoise-sigma") {
            ro.denoise_sigma = atof(need("--denoise-sigma")); denoise_knob_given = true;
            if (!(ro.denoise_sigma > 0.0)) { fprintf(stderr, "--denoise-sigma needs a width above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--denoise-albedo") ro.denoise = ro.denoise_albedo = true;
        else if (a == "--denoise-albedo-sigma") {
            ro.denoise_albedo_sigma = atof(need("--denoise-albedo-sigma")); albedo_knob_given = true;
            if (!(ro.denoise_albedo_sigma > 0.0)) { fprintf(stderr, "--denoise-albedo-sigma needs a width above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--denoise-edges") ro.denoise = ro.denoise_edges = true;
        else if (a == "--denoise-edges-sigma") {
            ro.denoise_edges_sigma = atof(need("--denoise-edges-sigma")); edges_knob_given = true;
            if (!(ro.denoise_edges_sigma > 0.0)) { fprintf(stderr, "--denoise-edges-sigma needs a width above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--live-denoise") ro.live_denoise = true;
        else if (a == "--live-denoise-albedo") ro.live_denoise = ro.live_denoise_albedo = true;
        else if (a == "--live-denoise-edges") ro.live_denoise = ro.live_denoise_edges = true;
        else if (a == "--live-denoise-spatial") {
            ro.live_denoise_spatial = 2; // N is optional: a following word that is a number is N
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') ro.live_denoise_spatial = atoi(argv[++i]);
            if (ro.live_denoise_spatial < 1) { fprintf(stderr, "--live-denoise-spatial needs a number of samples of at least 1\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--denoise-spatial-radius") {
            ro.denoise_spatial_radius = atoi(need("--denoise-spatial-radius")); spatial_knob_given = true;
            if (ro.denoise_spatial_radius < 1 || ro.denoise_spatial_radius > 3) { fprintf(stderr, "--denoise-spatial-radius needs a radius from 1 to 3\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--orbit") {
            ro.orbit = atoi(need("--orbit"));
            if (ro.orbit < 1 || ro.orbit > 1000) { fprintf(stderr, "--orbit needs a number of views from 1 to 1000\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--orbit-denoise") ro.orbit_denoise = true;
        else if (a == "--orbit-denoise-albedo") ro.orbit_denoise_albedo = true;
        else if (a == "--orbit-denoise-edges") ro.orbit_denoise_edges = true;
        else if (a == "--tonemap") {
            const std::string op = need("--tonemap");
            tonemap_given = true;
            if (op == "clamp") ro.tonemap = RT_TONEMAP_CLAMP;
            else if (op == "reinhard") ro.tonemap = RT_TONEMAP_REINHARD;
            else if (op == "aces") ro.tonemap = RT_TONEMAP_ACES;
            else { fprintf(stderr, "--tonemap needs an operator: clamp, reinhard or aces\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--exposure") {
            char *end = nullptr;
            const char *v = need("--exposure");
            ro.exposure_ev = strtod(v, &end); tonemap_given = true;
            if (end == v || *end != 0 || !(ro.exposure_ev >= -64.0 && ro.exposure_ev <= 64.0)) { fprintf(stderr, "--exposure needs a number of stops from -64 to 64\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--auto-exposure") {
            ro.auto_exposure = 0.18; tonemap_given = true; // KEY is optional: a following word that is a number is KEY
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) ro.auto_exposure = atof(argv[++i]);
            if (!(ro.auto_exposure > 0.0) || !(ro.auto_exposure < 1e300)) { fprintf(stderr, "--auto-exposure needs a key above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--tonemap-white") {
            ro.tonemap_white = atof(need("--tonemap-white")); tonemap_given = white_given = true;
            if (!(ro.tonemap_white > 0.0)) { fprintf(stderr, "--tonemap-white needs a value above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--bloom") {
            ro.bloom = 0.25; // STRENGTH is optional: a following word that is a number is STRENGTH
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) ro.bloom = atof(argv[++i]);
            if (!(ro.bloom >= 0.0) || !(ro.bloom < 1e300)) { fprintf(stderr, "--bloom needs a strength of at least 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--bloom-threshold") {
            char *end = nullptr;
            const char *v = need("--bloom-threshold");
            ro.bloom_threshold = strtod(v, &end); bloom_knob_given = true;
            if (end == v || *end != 0 || !(ro.bloom_threshold >= 0.0) || !(ro.bloom_threshold < 1e300)) { fprintf(stderr, "--bloom-threshold needs a luminance of at least 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--bloom-levels") {
            ro.bloom_levels = atoi(need("--bloom-levels")); bloom_knob_given = true;
            if (ro.bloom_levels < 1 || ro.bloom_levels > 8) { fprintf(stderr, "--bloom-levels needs a number of levels from 1 to 8\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--upsample") {
            char *end = nullptr;
            const char *v = need("--upsample");
            const long f = strtol(v, &end, 10);
            if (end == v || *end != 0 || f < 2 || f > 4) { fprintf(stderr, "--upsample needs a factor of 2, 3 or 4\n"); usage(argv[0]); return 2; }
            ro.upsample = (int)f;
        }
        else if (a == "--robust") {
            char *end = nullptr;
            const char *v = need("--robust");
            const long k = strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 1 || k > RT_ROBUST_MAX_BLOCKS) { fprintf(stderr, "--robust needs a number of blocks from 1 to 32\n"); usage(argv[0]); return 2; }
            ro.robust_blocks = (int)k;
        }
        else if (a == "--robust-mode") {
            const std::string m = need("--robust-mode");
            robust_knob_given = true;
            if (m == "mean") ro.robust_mode = RT_ROBUST_MEAN;
            else if (m == "trim") ro.robust_mode = RT_ROBUST_TRIM;
            else if (m == "median") ro.robust_mode = RT_ROBUST_MEDIAN;
            else if (m == "gini") ro.robust_mode = RT_ROBUST_GINI;
            else { fprintf(stderr, "--robust-mode needs a mode: mean, trim, median or gini\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--robust-trim") {
            char *end = nullptr;
            const char *v = need("--robust-trim");
            const long t = strtol(v, &end, 10);
            robust_knob_given = true;
            if (end == v || *end != 0 || t < 0 || t > RT_ROBUST_MAX_BLOCKS) { fprintf(stderr, "--robust-trim needs a number of values to drop at each end, from 0 to 32\n"); usage(argv[0]); return 2; }
            ro.robust_trim = (int)t;
        }
        else if (a == "--robust-gain") {
            char *end = nullptr;
            const char *v = need("--robust-gain");
            ro.robust_gain = strtod(v, &end); robust_knob_given = true;
            if (end == v || *end != 0 || !(ro.robust_gain > 0.0) || !(ro.robust_gain < 1e300)) { fprintf(stderr, "--robust-gain needs a gain above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--format") {
            const std::string f = need("--format");
            if (f == "png") ro.format = FILM_PNG;
            else if (f == "png16") ro.format = FILM_PNG16;
            else if (f == "hdr") ro.format = FILM_HDR;
            else if (f == "pfm") ro.format = FILM_PFM;
            else { fprintf(stderr, "--format needs a file format: png, png16, hdr or pfm\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--panorama") {
            char *end = nullptr;
            const char *v = need("--panorama");
            const long pw = strtol(v, &end, 10);
            if (end == v || *end != 0 || pw < 2 || pw > 32768 || pw % 2 != 0) { fprintf(stderr, "--panorama needs an even width from 2 to 32768\n"); usage(argv[0]); return 2; }
            ro.panorama_width = (int)pw;
        }
        else if (a == "--panorama-face") {
            char *end = nullptr;
            const char *v = need("--panorama-face");
            const long f = strtol(v, &end, 10);
            panorama_knob_given = true;
            if (end == v || *end != 0 || f < 2 || f > 16384) { fprintf(stderr, "--panorama-face needs a face size from 2 to 16384\n"); usage(argv[0]); return 2; }
            ro.panorama_face = (int)f;
        }
        else if (a == "--panorama-guard") {
            char *end = nullptr;
            const char *v = need("--panorama-guard");
            const long g = strtol(v, &end, 10);
            panorama_knob_given = true;
            if (end == v || *end != 0 || g < 0 || g > 8191) { fprintf(stderr, "--panorama-guard needs a number of guard texels from 0 to 8191\n"); usage(argv[0]); return 2; }
            ro.panorama_guard = (int)g;
        }
        else if (a == "--panorama-at") {
            const char *v = need("--panorama-at");
            char *end = nullptr;
            bool ok = true;
            panorama_knob_given = true;
            for (int c = 0; c < 3 && ok; ++c) {
                ro.panorama_at[c] = strtod(v, &end);
                ok = end != v && std::isfinite(ro.panorama_at[c]) && *end == (c < 2 ? ',' : 0);
                v = end + 1;
            }
            if (!ok) { fprintf(stderr, "--panorama-at needs a point x,y,z\n"); usage(argv[0]); return 2; }
            ro.panorama_at_given = true;
        }
        else if (a == "--compare") ro.compare_file = need("--compare");
        else if (a == "--compare-eps") {
            char *end = nullptr;
            const char *v = need("--compare-eps");
            ro.compare_eps = strtod(v, &end);
            compare_eps_given = true;
            if (end == v || *end != 0 || !(ro.compare_eps > 0.0) || !(ro.compare_eps < 1e300)) { fprintf(stderr, "--compare-eps needs a number above 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--live-stop") {
            char *end = nullptr;
            const char *v = need("--live-stop");
            ro.live_stop_noise = strtod(v, &end);
            if (end == v || *end != 0 || !(ro.live_stop_noise >= 0.0)) { fprintf(stderr, "--live-stop needs a noise threshold of at least 0\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--live-stop-min") {
            ro.live_stop_min_samples = atoi(need("--live-stop-min")); live_stop_min_given = true;
            if (ro.live_stop_min_samples < 1) { fprintf(stderr, "--live-stop-min needs a number of samples of at least 1\n"); usage(argv[0]); return 2; }
        }
        else if (a == "--upsample-albedo") ro.upsample_albedo = true;
        else if (a == "--upsample-edges") ro.upsample_edges = true;
        else if (a == "--earth") so.earth_image = need("--earth");
        else if (a == "--bvh") bvh_policy() = std::string(need("--bvh")) == "sah" ? BvhPolicy::Sah : BvhPolicy::Reference;
        else if (a == "-h" || a == "--help") { usage(argv[0]); return 0; }
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(argv[0]); return 2; }
    }
    printf("Args: { live: %s, scene: %d, output: \"%s\" }\n", live ? "true" : "false", scene, output.c_str());
    if (ro.adaptive && (ro.gpus > 1 || ro.progressive_spp > 0)) {
        fprintf(stderr, "--adaptive renders on one GPU in one pass: it cannot be combined with --gpus > 1 or --progressive\n");
        return 2;
    }
    if (ro.orbit > 0 && (ro.gpus > 1 || ro.progressive_spp > 0 || ro.adaptive)) {
        fprintf(stderr, "--orbit renders every view on one GPU in one launch: it cannot be combined with --gpus > 1, --progressive or --adaptive\n");
        usage(argv[0]);
        return 2;
    }
    if (live && (ro.gpus > 1 || ro.progressive_spp > 0 || ro.adaptive || ro.orbit > 0)) {
        fprintf(stderr, "--live refines one frame on one GPU: it cannot be combined with --gpus > 1, --progressive, --adaptive or --orbit\n");
        return 2;
    }
    if (ro.denoise && (live || ro.gpus > 1 || ro.progressive_spp > 0 || ro.orbit > 0)) {
        fprintf(stderr, "--denoise filters one frame's sums and sums of squares on one GPU: it cannot be combined with --live (a running mean keeps no "
                        "second moment), --gpus > 1 (the gather moves sums only), --progressive or --orbit\n");
        return 2;
    }
    if ((ro.orbit_denoise || ro.orbit_denoise_albedo) && ro.orbit == 0) {
        fprintf(stderr, "--orbit-denoise and --orbit-denoise-albedo filter the views of --orbit: they need --orbit\n");
        return 2;
    }
    if (ro.orbit_denoise_edges && ro.orbit == 0) {
        fprintf(stderr, "--orbit-denoise-edges guides the filter of the views of --orbit: it needs --orbit\n");
        return 2;
    }
    if (ro.live_denoise_edges && ro.upsample > 0) {
        fprintf(stderr, "--live-denoise-edges takes its surface-ID frame at the size it filters: it cannot be combined with --upsample (the guide "
                        "would have to be made at the low size)\n");
        return 2;
    }
    if (ro.orbit_denoise && ro.orbit_denoise_albedo) {
        fprintf(stderr, "--orbit-denoise and --orbit-denoise-albedo are two filters for the same views: give one of them\n");
        return 2;
    }
    if (ro.live_denoise && !live) {
        fprintf(stderr, "--live-denoise and --live-denoise-albedo filter the frames of --live: they need -l/--live\n");
        return 2;
    }
    if (ro.live_denoise_spatial > 0 && !ro.live_denoise) {
        fprintf(stderr, "--live-denoise-spatial sets how --live-denoise filters its first frames: it needs --live-denoise or --live-denoise-albedo\n");
        return 2;
    }
    if (spatial_knob_given && ro.live_denoise_spatial == 0) {
        fprintf(stderr, "--denoise-spatial-radius sets the window of --live-denoise-spatial: it needs --live-denoise-spatial\n");
        return 2;
    }
    if (albedo_knob_given && !ro.denoise_albedo && !ro.live_denoise_albedo && !ro.orbit_denoise_albedo) {
        fprintf(stderr, "--denoise-albedo-sigma sets the filter of --denoise-albedo: it needs --denoise-albedo (with --live: --live-denoise-albedo; "
                        "with --orbit: --orbit-denoise-albedo)\n");
        return 2;
    }
    if (edges_knob_given && !ro.denoise_edges && !ro.live_denoise_edges && !ro.orbit_denoise_edges) {
        fprintf(stderr, "--denoise-edges-sigma sets the filter of --denoise-edges: it needs --denoise-edges (with --live: --live-denoise-edges; "
                        "with --orbit: --orbit-denoise-edges)\n");
        return 2;
    }
    if (denoise_knob_given && !ro.denoise && !ro.live_denoise && !ro.orbit_denoise && !ro.orbit_denoise_albedo && !ro.orbit_denoise_edges) {
        fprintf(stderr, "--denoise-iters and --denoise-sigma set the filter of --denoise: they need --denoise (with --live: --live-denoise; "
                        "with --orbit: --orbit-denoise)\n");
        return 2;
    }
    if (tonemap_given && (ro.gpus > 1 || ro.progressive_spp > 0)) {
        fprintf(stderr, "--tonemap, --exposure, --auto-exposure and --tonemap-white shape the final bytes of a one-GPU, one-pass route: they cannot be "
                        "combined with --gpus > 1 or --progressive\n");
        return 2;
    }
    if (ro.bloom >= 0.0 && (ro.gpus > 1 || ro.progressive_spp > 0)) {
        fprintf(stderr, "--bloom runs in front of the tone mapping of a one-GPU, one-pass route: it cannot be combined with --gpus > 1 or --progressive\n");
        return 2;
    }
    if (ro.format != FILM_PNG && ro.gpus > 1) {
        fprintf(stderr, "--format other than png is written by the film stage of a one-GPU route: it cannot be combined with --gpus > 1 (the gather "
                        "carries 8-bit tiles)\n");
        return 2;
    }
    if (ro.format != FILM_PNG && ro.progressive_spp > 0) {
        fprintf(stderr, "--format other than png is written by the film stage of a one-pass route: it cannot be combined with --progressive (the "
                        "passes rewrite an 8-bit PNG)\n");
        return 2;
    }
    if (bloom_knob_given && ro.bloom < 0.0) {
        fprintf(stderr, "--bloom-threshold and --bloom-levels set the glow of --bloom: they need --bloom\n");
        return 2;
    }
    if ((ro.upsample_albedo || ro.upsample_edges) && ro.upsample == 0) {
        fprintf(stderr, "--upsample-albedo and --upsample-edges are the guides of --upsample: they need --upsample\n");
        return 2;
    }
    if (ro.upsample > 0 && (ro.orbit > 0 || ro.adaptive || ro.gpus > 1 || ro.progressive_spp > 0)) {
        fprintf(stderr, "--upsample traces a smaller frame on a one-GPU route — a plain render, the --denoise family or -l/--live: it cannot be "
                        "combined with --orbit, --adaptive, --gpus > 1 or --progressive\n");
        return 2;
    }
    if (robust_knob_given && ro.robust_blocks == 0) {
        fprintf(stderr, "--robust-mode, --robust-trim and --robust-gain set the combiner of --robust: they need --robust\n");
        return 2;
    }
    if (ro.robust_blocks > 0) {
        const char *with = live ? "-l/--live" : ro.adaptive ? "--adaptive" : ro.orbit > 0 ? "--orbit" : ro.progressive_spp > 0 ? "--progressive"
                           : ro.upsample > 0 ? "--upsample" : ro.gpus > 1 ? "--gpus > 1" : ro.denoise_albedo ? "--denoise-albedo"
                           : ro.denoise_edges ? "--denoise-edges" : nullptr;
        if (with) {
            fprintf(stderr, "--robust renders its sub-frames on one GPU in one launch and filters them with the plain --denoise only: it cannot be "
                            "combined with %s\n", with);
            return 2;
        }
    }
    if (panorama_knob_given && ro.panorama_width == 0) {
        fprintf(stderr, "--panorama-face, --panorama-guard and --panorama-at set the cube map of --panorama: they need --panorama\n");
        return 2;
    }
    if (ro.panorama_width > 0) {
        const char *with = live ? "-l/--live" : ro.adaptive ? "--adaptive" : ro.orbit > 0 ? "--orbit" : ro.progressive_spp > 0 ? "--progressive"
                           : ro.upsample > 0 ? "--upsample" : ro.robust_blocks > 0 ? "--robust" : ro.gpus > 1 ? "--gpus > 1"
                           : ro.denoise_albedo ? "--denoise-albedo" : ro.denoise_edges ? "--denoise-edges" : ro.denoise ? "--denoise" : nullptr;
        if (with) {
            fprintf(stderr, "--panorama renders its six cube faces on one GPU in one launch and resamples them unfiltered: it cannot be combined "
                            "with %s\n", with);
            return 2;
        }
    }
    if (white_given && ro.tonemap != RT_TONEMAP_REINHARD) {
        fprintf(stderr, "--tonemap-white sets the white point of --tonemap reinhard: it needs --tonemap reinhard\n");
        return 2;
    }
    if ((tonemap_given || ro.bloom >= 0.0) && ro.tonemap < 0) ro.tonemap = RT_TONEMAP_CLAMP; // an exposure or bloom alone: the stage with the plain clamp
    if (!ro.compare_file.empty() && (live || ro.orbit > 0 || ro.progressive_spp > 0 || ro.gpus > 1)) {
        const char *with = live ? "-l/--live" : ro.orbit > 0 ? "--orbit" : ro.progressive_spp > 0 ? "--progressive" : "--gpus > 1";
        fprintf(stderr, "--compare measures the one frame of a one-GPU, one-pass route against a reference: it cannot be combined with %s\n", with);
        return 2;
    }
    if (compare_eps_given && ro.compare_file.empty()) {
        fprintf(stderr, "--compare-eps sets the relative error's eps of --compare: it needs --compare\n");
        return 2;
    }
    if (ro.live_stop_noise >= 0.0 && !live) {
        fprintf(stderr, "--live-stop ends the passes of --live: it needs -l/--live\n");
        return 2;
    }
    if (live_stop_min_given && ro.live_stop_noise < 0.0) {
        fprintf(stderr, "--live-stop-min sets the fewest samples of --live-stop: it needs --live-stop\n");
        return 2;
    }
    if (live_spp_given && !live) {
        fprintf(stderr, "--live-spp sets the samples per frame of --live: it needs -l/--live\n");
        return 2;
    }
    if (live && !output_given) {
        fprintf(stderr, "--live has no window to draw in and writes its last frame to a file instead: name it with -o/--output\n");
        return 2;
    }

    try {
        seed_rng(scene_seed);
        auto [world, camera] = build_scene(scene, so);

        auto now = std::chrono::steady_clock::now();
        auto bvh = std::make_shared<BVHNode>(world);
        printf("Building BVH: %.2fms\n",
               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - now).count());

        if (live) {
            now = std::chrono::steady_clock::now();
            int frames = 0, samples = 0;
            std::vector<uint8_t> film;
            const std::vector<uint8_t> rgba = live_render(camera, *bvh, ro, [&](const std::vector<uint8_t> &, int n) { ++frames; samples = n; }, &film);
            printf("Live: %d frames, %d samples per pixel in the last, %.2fs\n", frames, samples,
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - now).count());
            if (ro.format != FILM_PNG) { // the last frame in the film format, from the means it was shown from
                write_film_frame(output, (int32_t)camera.image_width, (int32_t)camera.image_height, film, ro);
                return 0;
            }
            std::vector<uint8_t> rgb(rgba.size() / 4u * 3u);
            for (size_t p = 0; p < rgba.size() / 4u; ++p) { rgb[3 * p] = rgba[4 * p]; rgb[3 * p + 1] = rgba[4 * p + 1]; rgb[3 * p + 2] = rgba[4 * p + 2]; }
            if (!write_png_rgb8(output + ".png", (int32_t)camera.image_width, (int32_t)camera.image_height, rgb.data()))
                throw std::runtime_error("Should've encoded the image into a file.");
            return 0;
        }
        render(std::make_shared<Camera>(camera), bvh, output, ro);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
