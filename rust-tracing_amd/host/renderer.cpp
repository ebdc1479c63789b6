#include "renderer.hpp"
#include "color.hpp"
#include "image_io.hpp"
#include "rt_amd.h"
#include "rt_host.h"
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace rt {

std::vector<double> render_sums(const Camera &camera, const Hittable &world, const RenderOptions &opt,
                                const std::function<void(const std::vector<double> &, int)> &on_pass) {
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const rt_camera cam = camera.pod();

    const int ngpu = opt.gpus < 1 ? 1 : opt.gpus;
    if (rt_device_count() < ngpu)
        throw std::runtime_error("render: " + std::to_string(ngpu) + " GPU(s) requested, " +
                                 std::to_string(rt_device_count()) + " visible");

    std::vector<rt_scene *> scenes((size_t)ngpu, nullptr);
    auto destroy_all = [&]() { for (rt_scene *s : scenes) rt_scene_destroy(s); };
    for (int g = 0; g < ngpu; ++g)
        if (rt_scene_create(&desc, g, &scenes[(size_t)g]) != RT_OK) {
            const std::string msg = rt_last_error();
            destroy_all();
            throw std::runtime_error("render: " + msg);
        }

    std::vector<double> sums((size_t)cam.image_width * (size_t)cam.image_height * 3u, 0.0);
    const int spp = cam.samples_per_pixel;
    const int pass = opt.progressive_spp > 0 ? opt.progressive_spp : spp;
    const int32_t w = cam.image_width, h = cam.image_height;

    // Device route (include/rt_amd.h "frame-end gather"): every device renders its tiles (k % ngpu == g) into its own tile buffer in
    // HBM; at the end of a pass ONE grouped RCCL exchange brings the buffers to device 0 over xGMI, which reassembles the frame and
    // hands it to the host in one copy.  If RCCL cannot be loaded the frame travels through host memory instead (below).
    std::vector<rt_comm *> comms((size_t)ngpu, nullptr);
    // (one GPU: nothing to gather — no communicator, no RCCL: the frame comes back through rt_render's own copy, below)
    const bool device_route = ngpu > 1 && rt_comm_create_all(ngpu, nullptr, comms.data()) == RT_OK;
    if (device_route) {
        const int64_t stride = rt_out_size(w, h, RT_OUT_TILES, 0, ngpu);
        std::vector<void *> tiles((size_t)ngpu, nullptr);
        void *gathered = nullptr, *frame = nullptr;
        auto cleanup = [&]() {
            for (int g = 0; g < ngpu; ++g) { rt_device_free(g, tiles[(size_t)g]); rt_comm_destroy(comms[(size_t)g]); }
            rt_device_free(0, gathered); rt_device_free(0, frame);
            destroy_all();
        };
        bool ok = rt_device_malloc(0, stride * ngpu * (int64_t)sizeof(double), &gathered) == RT_OK &&
                  rt_device_malloc(0, (int64_t)sums.size() * (int64_t)sizeof(double), &frame) == RT_OK;
        for (int g = 0; g < ngpu && ok; ++g) ok = rt_device_malloc(g, stride * (int64_t)sizeof(double), &tiles[(size_t)g]) == RT_OK;
        if (!ok) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); }
        for (int begin = 0; begin < spp; begin += pass) {
            const int end = begin + pass < spp ? begin + pass : spp;
            std::vector<std::string> errors((size_t)ngpu);
            auto on_every_device = [&](auto &&fn) { // one host thread per device
                std::vector<std::thread> workers;
                for (int g = 0; g < ngpu; ++g) workers.emplace_back([&, g]() { if (fn(g) != RT_OK) errors[(size_t)g] = rt_last_error(); });
                for (auto &t : workers) t.join();
                for (const auto &e : errors)
                    if (!e.empty()) { cleanup(); throw std::runtime_error("render: " + e); }
            };
            // Two phases with a join in between: a rank enters the grouped exchange only when EVERY rank has rendered — a rank that
            // failed and stayed out would leave its peers' ncclSend / ncclRecv pending for ever (and cleanup() waiting on them).
            on_every_device([&](int g) {
                rt_render_params p{};
                p.seed = opt.seed; p.sample_begin = begin; p.sample_end = end; p.max_depth = cam.max_depth;
                p.accumulate = begin > 0 ? 1 : 0; // the tile buffers keep the running sums between passes
                p.shard_index = g; p.shard_count = ngpu; p.out_layout = RT_OUT_TILES; p.device = g;
                return rt_render_device(scenes[(size_t)g], &cam, &p, static_cast<double *>(tiles[(size_t)g]), nullptr);
            });
            on_every_device([&](int g) {
                return rt_gather_tiles_device(comms[(size_t)g], w, h, 8, tiles[(size_t)g], g == 0 ? gathered : nullptr, 0, nullptr);
            });
            if (rt_tiles_to_frame_device(w, h, ngpu, static_cast<const double *>(gathered), static_cast<double *>(frame), nullptr) != RT_OK ||
                rt_device_download(0, sums.data(), frame, (int64_t)sums.size() * (int64_t)sizeof(double), nullptr) != RT_OK) {
                const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg);
            }
            if (on_pass) on_pass(sums, end);
        }
        cleanup();
        return sums;
    }

    for (int begin = 0; begin < spp; begin += pass) {
        const int end = begin + pass < spp ? begin + pass : spp;
        std::vector<std::string> errors((size_t)ngpu);
        std::vector<std::thread> workers;
        // one host thread per device; each renders the tiles k with k % ngpu == g into its own pixels of `sums`
        for (int g = 0; g < ngpu; ++g) {
            workers.emplace_back([&, g]() {
                rt_render_params p{};
                p.seed = opt.seed;
                p.sample_begin = begin;
                p.sample_end = end;
                p.max_depth = cam.max_depth;
                p.accumulate = begin > 0 ? 1 : 0;
                p.shard_index = g;
                p.shard_count = ngpu;
                p.out_layout = RT_OUT_FRAME;
                p.device = g;
                if (rt_render(scenes[(size_t)g], &cam, &p, sums.data()) != RT_OK) errors[(size_t)g] = rt_last_error();
            });
        }
        for (auto &w : workers) w.join();
        for (const auto &e : errors)
            if (!e.empty()) {
                destroy_all();
                throw std::runtime_error("render: " + e);
            }
        if (on_pass) on_pass(sums, end);
    }
    destroy_all();
    return sums;
}

std::vector<uint8_t> resolve_rgb8(const std::vector<double> &sums, int32_t spp) {
    std::vector<uint8_t> px(sums.size());
    const FP inv = 1.0 / (FP)spp; // `c / spp as FP` is a multiply by the reciprocal (src/vec3.rs:244-249)
    for (size_t i = 0; i + 2 < sums.size(); i += 3) {
        const auto rgb = color_to_rgb(Color(sums[i] * inv, sums[i + 1] * inv, sums[i + 2] * inv));
        px[i] = rgb[0]; px[i + 1] = rgb[1]; px[i + 2] = rgb[2];
    }
    return px;
}

// The tone-mapping stage (include/rt_amd.h "tone mapping") is on when any of its options was given: opt.tonemap >= 0 — or when bloom
// is on (opt.bloom >= 0), which runs in front of it: the stage then has the clamp unless an operator was chosen.
// A film format (opt.format other than FILM_PNG; include/rt_amd.h "film output") turns the stage on as well: the film stage is the
// tone-mapping stage with another last step, and with nothing else given it runs with the clamp and exposure 1, where its value is the mean.
static bool filmed(const RenderOptions &opt) { return opt.format != FILM_PNG; }
static bool tonemapped(const RenderOptions &opt) { return opt.tonemap >= 0 || opt.bloom >= 0.0 || filmed(opt); }
static rt_tonemap_params tonemap_params(const char *who, const RenderOptions &opt) {
    rt_tonemap_params tp;
    if (rt_tonemap_params_init_sized(&tp, sizeof tp) != RT_OK) throw std::runtime_error(std::string(who) + ": " + rt_last_error());
    tp.op = opt.tonemap >= 0 ? opt.tonemap : RT_TONEMAP_CLAMP; tp.exposure = std::exp2(opt.exposure_ev); tp.auto_key = opt.auto_exposure; tp.white = opt.tonemap_white;
    return tp;
}

std::vector<uint8_t> tonemap_rgb8(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt) {
    const rt_tonemap_params tp = tonemap_params("tonemap", opt);
    std::vector<uint8_t> px((size_t)width * (size_t)height * 3u);
    if (values.size() != px.size()) throw std::runtime_error("tonemap: the frame does not hold 3 * width * height values");
    if (rth_tonemap(width, height, values.data(), spp, nullptr, &tp, px.data(), nullptr) != 0) throw std::runtime_error(rth_last_error());
    return px;
}

std::vector<uint8_t> tonemap_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, bool rgba,
                                    const RenderOptions &opt) {
    const rt_tonemap_params tp = tonemap_params("tonemap", opt);
    const int64_t n_pix = (int64_t)width * height, bytes = n_pix * (rgba ? 4 : 3), work = rt_tonemap_workspace_bytes(width, height);
    void *d_out = nullptr, *d_work = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_out); rt_device_free(0, d_work); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("tonemap: " + msg); } };
    if (work < 0) throw std::runtime_error("tonemap: no workspace for a frame of this size");
    check(rt_device_malloc(0, bytes, &d_out));
    if (tp.auto_key > 0.0) check(rt_device_malloc(0, work, &d_work));
    check(rt_tonemap_device(width, height, d_values, spp, d_spp, &tp, rgba ? nullptr : static_cast<uint8_t *>(d_out),
                            rgba ? static_cast<uint8_t *>(d_out) : nullptr, d_work, nullptr));
    std::vector<uint8_t> px((size_t)bytes);
    check(rt_device_download(0, px.data(), d_out, bytes, nullptr)); // (waits for the stage: the buffers are freed behind it)
    cleanup();
    return px;
}

// The film stage with opt's operator, exposure, key and white, in the format opt.format's file takes.
static int32_t film_format(const RenderOptions &opt) { return opt.format == FILM_HDR ? RT_FILM_RGBE : opt.format == FILM_PFM ? RT_FILM_F32 : RT_FILM_RGB16; }

std::vector<uint8_t> film_host(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt) {
    const rt_tonemap_params tp = tonemap_params("film", opt);
    const int64_t bytes = rt_film_bytes(width, height, film_format(opt));
    if (bytes < 0) throw std::runtime_error("film: no frame of this size");
    if (values.size() != (size_t)width * (size_t)height * 3u) throw std::runtime_error("film: the frame does not hold 3 * width * height values");
    std::vector<uint8_t> px((size_t)bytes);
    if (rth_film(width, height, values.data(), spp, nullptr, &tp, film_format(opt), px.data()) != 0) throw std::runtime_error(rth_last_error());
    return px;
}

std::vector<uint8_t> film_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const RenderOptions &opt) {
    const rt_tonemap_params tp = tonemap_params("film", opt);
    const int64_t bytes = rt_film_bytes(width, height, film_format(opt)), work = rt_tonemap_workspace_bytes(width, height);
    void *d_out = nullptr, *d_work = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_out); rt_device_free(0, d_work); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("film: " + msg); } };
    if (bytes < 0 || work < 0) throw std::runtime_error("film: no frame of this size");
    check(rt_device_malloc(0, bytes, &d_out));
    if (tp.auto_key > 0.0) check(rt_device_malloc(0, work, &d_work));
    check(rt_film_device(width, height, d_values, spp, d_spp, &tp, film_format(opt), d_out, d_work, nullptr));
    std::vector<uint8_t> px((size_t)bytes);
    check(rt_device_download(0, px.data(), d_out, bytes, nullptr)); // (waits for the stage: the buffers are freed behind it)
    cleanup();
    return px;
}

// Bloom (include/rt_amd.h "bloom") is on when opt.bloom >= 0; it runs in front of the tone-mapping stage, which then takes means.
static bool bloomed(const RenderOptions &opt) { return opt.bloom >= 0.0; }
static rt_bloom_params bloom_params(const RenderOptions &opt) {
    rt_bloom_params bp;
    if (rt_bloom_params_init_sized(&bp, sizeof bp) != RT_OK) throw std::runtime_error(std::string("bloom: ") + rt_last_error());
    bp.levels = opt.bloom_levels; bp.threshold = opt.bloom_threshold; bp.strength = opt.bloom;
    return bp;
}

std::vector<double> bloom_means(const std::vector<double> &values, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt) {
    const rt_bloom_params bp = bloom_params(opt);
    std::vector<double> out((size_t)width * (size_t)height * 3u);
    if (values.size() != out.size()) throw std::runtime_error("bloom: the frame does not hold 3 * width * height values");
    if (rth_bloom(width, height, values.data(), spp, nullptr, &bp, out.data()) != 0) throw std::runtime_error(rth_last_error());
    return out;
}

void bloom_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, double *d_mean_out, const RenderOptions &opt) {
    const rt_bloom_params bp = bloom_params(opt);
    const int64_t work = rt_bloom_workspace_bytes(width, height);
    if (work < 0) throw std::runtime_error("bloom: no workspace for a frame of this size");
    void *d_work = nullptr;
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); rt_device_free(0, d_work); throw std::runtime_error("bloom: " + msg); } };
    check(rt_device_malloc(0, work, &d_work));
    check(rt_bloom_device(width, height, d_values, spp, d_spp, &bp, d_mean_out, d_work, nullptr));
    double first = 0.0; // (a download waits for everything enqueued before it: the workspace is freed behind the call)
    check(rt_device_download(0, &first, d_mean_out, (int64_t)sizeof first, nullptr));
    rt_device_free(0, d_work);
}

// the output stage of a HOST frame of sums when the tone-mapping stage is on: bloom first if it is on, then the stage on its means —
// or, with a film format, the film stage in its place: the bytes are then the frame in that format, what write_frame takes
static std::vector<uint8_t> staged_rgb8(const std::vector<double> &sums, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt) {
    const auto stage = filmed(opt) ? film_host : tonemap_rgb8;
    if (!bloomed(opt)) return stage(sums, width, height, spp, opt);
    return stage(bloom_means(sums, width, height, spp, opt), width, height, 1, opt);
}

// ... and of a DEVICE frame
static std::vector<uint8_t> staged_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, bool rgba,
                                          const RenderOptions &opt) {
    auto stage = [&](const double *d_frame, int32_t n, const int32_t *d_map) { // (a film format has one layout: `rgba` is the display bytes' choice)
        return filmed(opt) ? film_device(width, height, d_frame, n, d_map, opt) : tonemap_device(width, height, d_frame, n, d_map, rgba, opt);
    };
    if (!bloomed(opt)) return stage(d_values, spp, d_spp);
    void *d_bloomed = nullptr;
    if (rt_device_malloc(0, (int64_t)width * height * 3 * (int64_t)sizeof(double), &d_bloomed) != RT_OK) throw std::runtime_error(std::string("bloom: ") + rt_last_error());
    std::vector<uint8_t> px;
    try {
        bloom_device(width, height, d_values, spp, d_spp, static_cast<double *>(d_bloomed), opt);
        px = stage(static_cast<const double *>(d_bloomed), 1, nullptr);
    } catch (...) { rt_device_free(0, d_bloomed); throw; }
    rt_device_free(0, d_bloomed);
    return px;
}

// Frame metrics (include/rt_amd.h "frame metrics") on device 0: the output and the workspace are allocated here, the call is waited for
// (the download of its doubles) and both are freed behind it.
void frame_error_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const double *d_ref, int32_t ref_spp,
                        double eps, double out8[8]) {
    rt_frame_error_params ep;
    if (rt_frame_error_params_init_sized(&ep, sizeof ep) != RT_OK) throw std::runtime_error(std::string("frame_error: ") + rt_last_error());
    if (eps > 0.0) ep.eps = eps;
    const int64_t work = rt_metrics_workspace_bytes(width, height);
    if (work < 0) throw std::runtime_error("frame_error: no workspace for a frame of this size");
    void *d_out = nullptr, *d_work = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_out); rt_device_free(0, d_work); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("frame_error: " + msg); } };
    check(rt_device_malloc(0, 8 * (int64_t)sizeof(double), &d_out));
    check(rt_device_malloc(0, work, &d_work));
    check(rt_frame_error_device(width, height, d_values, spp, d_spp, d_ref, ref_spp, &ep, static_cast<double *>(d_out), d_work, nullptr));
    check(rt_device_download(0, out8, d_out, 8 * (int64_t)sizeof(double), nullptr));
    cleanup();
}

void frame_noise_device(int32_t width, int32_t height, int32_t form, const double *d_a, const double *d_b, int32_t n, const int32_t *d_spp, double eps,
                        double out4[4]) {
    rt_frame_noise_params np;
    if (rt_frame_noise_params_init_sized(&np, sizeof np) != RT_OK) throw std::runtime_error(std::string("frame_noise: ") + rt_last_error());
    if (eps > 0.0) np.eps = eps;
    const int64_t work = rt_metrics_workspace_bytes(width, height);
    if (work < 0) throw std::runtime_error("frame_noise: no workspace for a frame of this size");
    void *d_out = nullptr, *d_work = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_out); rt_device_free(0, d_work); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("frame_noise: " + msg); } };
    check(rt_device_malloc(0, 4 * (int64_t)sizeof(double), &d_out));
    check(rt_device_malloc(0, work, &d_work));
    check(rt_frame_noise_device(width, height, form, d_a, d_b, n, d_spp, &np, static_cast<double *>(d_out), d_work, nullptr));
    check(rt_device_download(0, out4, d_out, 4 * (int64_t)sizeof(double), nullptr));
    cleanup();
}

// opt.compare_file: the reference frame (means) of a w x h route, and the one line render() prints of a frame's eight values
static bool compared(const RenderOptions &opt) { return !opt.compare_file.empty(); }
static std::vector<double> compare_reference(int32_t width, int32_t height, const RenderOptions &opt) {
    int32_t rw = 0, rh = 0;
    std::vector<double> ref;
    const std::string bad = read_pfm_rgb(opt.compare_file, rw, rh, &ref);
    if (!bad.empty()) throw std::runtime_error("render: compare_file: " + bad);
    if (rw != width || rh != height)
        throw std::runtime_error("render: compare_file holds a " + std::to_string(rw) + " x " + std::to_string(rh) + " frame, the render a " +
                                 std::to_string(width) + " x " + std::to_string(height) + " one");
    return ref;
}
static void print_metrics(const double m[8]) {
    printf("metrics: count=%.17g mse=%.17g rmse=%.17g relmse=%.17g mae=%.17g bias=%.17g max=%.17g psnr=%.17g\n", m[0], m[1], m[2], m[3], m[4], m[5], m[6],
           m[7]);
}
// the values a route's output stage is about to read, against the reference: a HOST frame of sums through the mirror ...
static void compare_host(const std::vector<double> &sums, int32_t width, int32_t height, int32_t spp, const RenderOptions &opt) {
    if (!compared(opt)) return;
    const std::vector<double> ref = compare_reference(width, height, opt);
    rt_frame_error_params ep;
    if (rt_frame_error_params_init_sized(&ep, sizeof ep) != RT_OK) throw std::runtime_error(std::string("render: ") + rt_last_error());
    if (opt.compare_eps > 0.0) ep.eps = opt.compare_eps;
    double m[8];
    if (rth_frame_error(width, height, sums.data(), spp, nullptr, ref.data(), 1, &ep, m) != 0) throw std::runtime_error(std::string("render: ") + rth_last_error());
    print_metrics(m);
}
// ... and a DEVICE frame (sums with spp or a device map; means with spp = 1) through rt_frame_error_device
static void compare_device(int32_t width, int32_t height, const double *d_values, int32_t spp, const int32_t *d_spp, const RenderOptions &opt) {
    if (!compared(opt)) return;
    const std::vector<double> ref = compare_reference(width, height, opt);
    const int64_t bytes = (int64_t)ref.size() * (int64_t)sizeof(double);
    void *d_ref = nullptr;
    if (rt_device_malloc(0, bytes, &d_ref) != RT_OK) throw std::runtime_error(std::string("render: ") + rt_last_error());
    double m[8];
    try {
        if (rt_device_upload(0, d_ref, ref.data(), bytes, nullptr) != RT_OK) throw std::runtime_error(std::string("render: ") + rt_last_error());
        frame_error_device(width, height, d_values, spp, d_spp, static_cast<const double *>(d_ref), 1, opt.compare_eps, m);
    } catch (...) { rt_device_free(0, d_ref); throw; }
    rt_device_free(0, d_ref);
    print_metrics(m);
}

// The frame's file: NAME.png from RGB bytes, or with a film format NAME.hdr / NAME.pfm / NAME.png from the bytes the staging made in it.
static void write_frame(const std::string &name, int32_t width, int32_t height, const std::vector<uint8_t> &px, const RenderOptions &opt) {
    const int64_t want = filmed(opt) ? rt_film_bytes(width, height, film_format(opt)) : (int64_t)width * height * 3;
    bool ok = want >= 0 && px.size() >= (size_t)want;
    if (!ok) throw std::runtime_error("render: the frame's bytes do not fit its format");
    switch (opt.format) {
    case FILM_HDR: ok = write_hdr_rgbe(name + ".hdr", width, height, px.data()); break;
    case FILM_PFM: ok = write_pfm_rgb(name + ".pfm", width, height, reinterpret_cast<const float *>(px.data())); break;
    case FILM_PNG16: ok = write_png_rgb16(name + ".png", width, height, reinterpret_cast<const uint16_t *>(px.data())); break;
    default: ok = write_png_rgb8(name + ".png", width, height, px.data()); break;
    }
    if (!ok) throw std::runtime_error("Should've encoded the image into a file."); // src/renderer.rs:72
}

void write_film_frame(const std::string &name, int32_t width, int32_t height, const std::vector<uint8_t> &film, const RenderOptions &opt) {
    write_frame(name, width, height, film, opt);
}

// Guided upsampling (include/rt_amd.h "guided upsampling") is on when opt.upsample is a factor, 2..4.
static rt_upsample_params upsample_params(const RenderOptions &opt) {
    rt_upsample_params up;
    if (rt_upsample_params_init_sized(&up, sizeof up) != RT_OK) throw std::runtime_error(std::string("upsample: ") + rt_last_error());
    up.factor = opt.upsample;
    return up;
}

std::vector<double> upsample_means(const std::vector<double> &low, int32_t width, int32_t height, int32_t spp, const std::vector<double> &albedo_sum,
                                   int32_t albedo_spp, const std::vector<double> &edge_sum, int32_t edge_spp, const RenderOptions &opt) {
    const rt_upsample_params up = upsample_params(opt);
    const size_t full = width > 0 && height > 0 ? (size_t)width * (size_t)height * 3u : 0u;
    const int32_t F = up.factor >= 2 && up.factor <= 4 ? up.factor : 2; // (a factor out of range is refused below, by the library)
    const size_t small = full ? (size_t)((width + F - 1) / F) * (size_t)((height + F - 1) / F) * 3u : 0u;
    if (low.size() != small || (!albedo_sum.empty() && albedo_sum.size() != full) || (!edge_sum.empty() && edge_sum.size() != full))
        throw std::runtime_error("upsample: a frame does not hold the values of its size");
    std::vector<double> out(full);
    if (rth_upsample(width, height, low.data(), spp, albedo_sum.empty() ? nullptr : albedo_sum.data(), albedo_spp,
                     edge_sum.empty() ? nullptr : edge_sum.data(), edge_spp, &up, out.data(), nullptr) != 0)
        throw std::runtime_error(rth_last_error());
    return out;
}

void upsample_device(int32_t width, int32_t height, const double *d_low, int32_t spp, const double *d_albedo_sum, int32_t albedo_spp,
                     const double *d_edge_sum, int32_t edge_spp, double *d_mean_out, const RenderOptions &opt) {
    const rt_upsample_params up = upsample_params(opt);
    const int64_t work = rt_upsample_workspace_bytes(width, height, up.factor);
    if (work < 0) throw std::runtime_error("upsample: no workspace for a frame of this size at this factor");
    void *d_work = nullptr;
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); rt_device_free(0, d_work); throw std::runtime_error("upsample: " + msg); } };
    check(rt_device_malloc(0, work, &d_work));
    check(rt_upsample_device(width, height, d_low, spp, d_albedo_sum, albedo_spp, d_edge_sum, edge_spp, &up, d_mean_out, nullptr, d_work, nullptr));
    double first = 0.0; // (a download waits for everything enqueued before it: the workspace is freed behind the call)
    check(rt_device_download(0, &first, d_mean_out, (int64_t)sizeof first, nullptr));
    rt_device_free(0, d_work);
}

// One description of a denoise request on device 0, behind every rt::denoise* below, live_render and the upsample route.
enum class DenoiseForm { Sums, Means, Views };   // Views: a stack of n_views frames of sums, one behind the other in every buffer
enum class DenoiseGuides { None, Albedo, Edge }; // Edge: rt_denoise_guided_*, with the albedo guide as well where its frame is not null
struct DenoiseRequest {
    DenoiseForm form;
    DenoiseGuides guides;
    int32_t width, height;
    const double *first, *second;     // sums and sums of squares, or running means and M2
    int32_t count;                    // spp, or samples
    const int32_t *spp_map = nullptr; // Sums only
    const double *albedo = nullptr;   // (the counts: Sums and Views only)
    int32_t albedo_count = 0;
    const double *edge = nullptr;
    int32_t edge_count = 0;
    bool spatial = false; // Means only: through the *_mean_spatial entry points
    int32_t n_views = 1;  // Views only
};

// the spatial route's params from the options (live_denoise_spatial 0: the library's threshold)
static int spatial_params(const RenderOptions &opt, rt_denoise_spatial_params *sp) {
    if (int rc = rt_denoise_spatial_params_init_sized(sp, sizeof *sp)) return rc;
    if (opt.live_denoise_spatial > 0) sp->spatial_below = opt.live_denoise_spatial;
    sp->window_radius = opt.denoise_spatial_radius;
    return RT_OK;
}

// the albedo-guided and the plain filter's params from the edge-guided one's: each struct is the next one's first fields
static_assert(offsetof(rt_denoise_albedo_params, sigma_albedo) == sizeof(rt_denoise_params) &&
              offsetof(rt_denoise_guided_params, sigma_edge) == sizeof(rt_denoise_albedo_params), "the denoise params structs extend one another");
template <class P> static P narrowed(const rt_denoise_guided_params &gp) {
    P p;
    memcpy(&p, &gp, sizeof p);
    p.struct_size = (uint32_t)sizeof p;
    return p;
}

// The request's workspace in bytes (-1: a size the library refuses), and the request itself into device buffers: the filter's params from
// the options, and the C entry point of the request's form and guides.  Returns the library's code; rt_last_error() has the text.
static int64_t denoise_workspace_bytes(const DenoiseRequest &r) {
    const bool views = r.form == DenoiseForm::Views;
    switch (r.guides) {
    case DenoiseGuides::None: return views ? rt_denoise_views_workspace_bytes(r.width, r.height, r.n_views) : rt_denoise_workspace_bytes(r.width, r.height);
    case DenoiseGuides::Albedo:
        return views ? rt_denoise_albedo_views_workspace_bytes(r.width, r.height, r.n_views) : rt_denoise_albedo_workspace_bytes(r.width, r.height);
    default:
        return views ? rt_denoise_guided_views_workspace_bytes(r.width, r.height, r.n_views, r.albedo != nullptr)
                     : rt_denoise_guided_workspace_bytes(r.width, r.height, r.albedo != nullptr);
    }
}
static int denoise_into(const DenoiseRequest &r, const RenderOptions &opt, double *d_out, uint8_t *d_rgba8, void *d_work) {
    rt_denoise_guided_params gp;
    if (int rc = rt_denoise_guided_params_init_sized(&gp, sizeof gp)) return rc;
    gp.iterations = opt.denoise_iters; gp.sigma = opt.denoise_sigma; gp.sigma_albedo = opt.denoise_albedo_sigma; gp.sigma_edge = opt.denoise_edges_sigma;
    const rt_denoise_albedo_params ap = narrowed<rt_denoise_albedo_params>(gp);
    const rt_denoise_params pp = narrowed<rt_denoise_params>(gp);
    rt_denoise_spatial_params sp{};
    if (r.spatial)
        if (int rc = spatial_params(opt, &sp)) return rc;
    const int32_t w = r.width, h = r.height, n = r.count;
    const double *A = r.albedo, *E = r.edge;
    switch (r.form) {
    case DenoiseForm::Sums:
        switch (r.guides) {
        case DenoiseGuides::None: return rt_denoise_device(w, h, r.first, r.second, n, r.spp_map, &pp, d_out, d_rgba8, d_work, nullptr);
        case DenoiseGuides::Albedo: return rt_denoise_albedo_device(w, h, r.first, r.second, n, r.spp_map, A, r.albedo_count, &ap, d_out, d_rgba8, d_work, nullptr);
        default: return rt_denoise_guided_device(w, h, r.first, r.second, n, r.spp_map, A, r.albedo_count, E, r.edge_count, &gp, d_out, d_rgba8, d_work, nullptr);
        }
    case DenoiseForm::Views:
        switch (r.guides) {
        case DenoiseGuides::None: return rt_denoise_views_device(w, h, r.n_views, r.first, r.second, n, &pp, d_out, d_rgba8, d_work, nullptr);
        case DenoiseGuides::Albedo:
            return rt_denoise_albedo_views_device(w, h, r.n_views, r.first, r.second, n, A, r.albedo_count, &ap, d_out, d_rgba8, d_work, nullptr);
        default:
            return rt_denoise_guided_views_device(w, h, r.n_views, r.first, r.second, n, A, r.albedo_count, E, r.edge_count, &gp, d_out, d_rgba8, d_work, nullptr);
        }
    default:
        switch (r.guides) {
        case DenoiseGuides::None:
            return r.spatial ? rt_denoise_mean_spatial_device(w, h, r.first, r.second, n, &sp, &pp, d_out, d_rgba8, d_work, nullptr)
                             : rt_denoise_mean_device(w, h, r.first, r.second, n, &pp, d_out, d_rgba8, d_work, nullptr);
        case DenoiseGuides::Albedo:
            return r.spatial ? rt_denoise_albedo_mean_spatial_device(w, h, r.first, r.second, n, A, &sp, &ap, d_out, d_rgba8, d_work, nullptr)
                             : rt_denoise_albedo_mean_device(w, h, r.first, r.second, n, A, &ap, d_out, d_rgba8, d_work, nullptr);
        default:
            return r.spatial ? rt_denoise_guided_mean_spatial_device(w, h, r.first, r.second, n, A, E, &sp, &gp, d_out, d_rgba8, d_work, nullptr)
                             : rt_denoise_guided_mean_device(w, h, r.first, r.second, n, A, E, &gp, d_out, d_rgba8, d_work, nullptr);
        }
    }
}

// what every rt::denoise* is: the output and the workspace on device 0, the request run into them, the display bytes back as RGB, every
// frame of a stack behind the one before.  With the tone-mapping stage on, the filter writes no bytes (a null d_rgba8) and the stage makes
// them from the filtered means, every frame of a stack as a frame of its own.
static std::vector<uint8_t> run_denoise(const char *who, const DenoiseRequest &r, const RenderOptions &opt) {
    const int32_t width = r.width, height = r.height, n_frames = r.n_views;
    if (n_frames < 1) throw std::runtime_error(std::string(who) + ": n_views must be at least 1");
    const int64_t n_pix = (int64_t)width * height * n_frames, work = denoise_workspace_bytes(r);
    void *d_mean = nullptr, *d_rgba8 = nullptr, *d_work = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_mean); rt_device_free(0, d_rgba8); rt_device_free(0, d_work); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error(std::string(who) + ": " + msg); } };
    if (work < 0) throw std::runtime_error(std::string(who) + ": no workspace for a frame of this size");
    check(rt_device_malloc(0, n_pix * 3 * (int64_t)sizeof(double), &d_mean));
    if (!tonemapped(opt)) check(rt_device_malloc(0, n_pix * 4, &d_rgba8));
    check(rt_device_malloc(0, work, &d_work));
    check(denoise_into(r, opt, static_cast<double *>(d_mean), static_cast<uint8_t *>(d_rgba8), d_work));
    if (compared(opt) && n_frames == 1) { // the filtered means, what the output stage reads
        try { compare_device(width, height, static_cast<const double *>(d_mean), 1, nullptr, opt); }
        catch (...) { cleanup(); throw; }
    }
    if (tonemapped(opt)) {
        std::vector<uint8_t> rgb;
        try {
            for (int32_t k = 0; k < n_frames; ++k) {
                const std::vector<uint8_t> one = staged_device(width, height, static_cast<const double *>(d_mean) + (int64_t)k * width * height * 3, 1,
                                                               nullptr, false, opt);
                rgb.insert(rgb.end(), one.begin(), one.end());
            }
        } catch (...) { cleanup(); throw; }
        cleanup();
        return rgb;
    }
    std::vector<uint8_t> rgba((size_t)n_pix * 4u);
    check(rt_device_download(0, rgba.data(), d_rgba8, n_pix * 4, nullptr));
    cleanup();
    std::vector<uint8_t> rgb((size_t)n_pix * 3u);
    for (size_t p = 0; p < (size_t)n_pix; ++p) { rgb[3 * p] = rgba[4 * p]; rgb[3 * p + 1] = rgba[4 * p + 1]; rgb[3 * p + 2] = rgba[4 * p + 2]; }
    return rgb;
}

std::vector<uint8_t> denoise(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                             const RenderOptions &opt) {
    return run_denoise("denoise", {.form = DenoiseForm::Sums, .guides = DenoiseGuides::None, .width = width, .height = height, .first = d_sum,
                                   .second = d_sum_sq, .count = spp, .spp_map = d_spp}, opt);
}

std::vector<uint8_t> denoise_albedo(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                                    const double *d_albedo_sum, int32_t albedo_spp, const RenderOptions &opt) {
    return run_denoise("denoise_albedo", {.form = DenoiseForm::Sums, .guides = DenoiseGuides::Albedo, .width = width, .height = height, .first = d_sum,
                                          .second = d_sum_sq, .count = spp, .spp_map = d_spp, .albedo = d_albedo_sum, .albedo_count = albedo_spp}, opt);
}

std::vector<uint8_t> denoise_guided(int32_t width, int32_t height, const double *d_sum, const double *d_sum_sq, int32_t spp, const int32_t *d_spp,
                                    const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp, const RenderOptions &opt) {
    return run_denoise("denoise_guided", {.form = DenoiseForm::Sums, .guides = DenoiseGuides::Edge, .width = width, .height = height, .first = d_sum,
                                          .second = d_sum_sq, .count = spp, .spp_map = d_spp, .albedo = d_albedo_sum, .albedo_count = albedo_spp,
                                          .edge = d_edge_sum, .edge_count = edge_spp}, opt);
}

std::vector<uint8_t> denoise_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                   const RenderOptions &opt) {
    return run_denoise("denoise_views", {.form = DenoiseForm::Views, .guides = DenoiseGuides::None, .width = width, .height = height, .first = d_sum,
                                         .second = d_sum_sq, .count = spp, .n_views = n_views}, opt);
}

std::vector<uint8_t> denoise_albedo_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                          const double *d_albedo_sum, int32_t albedo_spp, const RenderOptions &opt) {
    return run_denoise("denoise_albedo_views", {.form = DenoiseForm::Views, .guides = DenoiseGuides::Albedo, .width = width, .height = height,
                                                .first = d_sum, .second = d_sum_sq, .count = spp, .albedo = d_albedo_sum, .albedo_count = albedo_spp,
                                                .n_views = n_views}, opt);
}

std::vector<uint8_t> denoise_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples, const RenderOptions &opt) {
    return run_denoise("denoise_mean", {.form = DenoiseForm::Means, .guides = DenoiseGuides::None, .width = width, .height = height, .first = d_mean,
                                        .second = d_m2, .count = samples}, opt);
}

std::vector<uint8_t> denoise_albedo_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                         const double *d_albedo_mean, const RenderOptions &opt) {
    return run_denoise("denoise_albedo_mean", {.form = DenoiseForm::Means, .guides = DenoiseGuides::Albedo, .width = width, .height = height,
                                               .first = d_mean, .second = d_m2, .count = samples, .albedo = d_albedo_mean}, opt);
}

std::vector<uint8_t> denoise_mean_spatial(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                          const RenderOptions &opt) {
    return run_denoise("denoise_mean_spatial", {.form = DenoiseForm::Means, .guides = DenoiseGuides::None, .width = width, .height = height,
                                                .first = d_mean, .second = d_m2, .count = samples, .spatial = true}, opt);
}

std::vector<uint8_t> denoise_albedo_mean_spatial(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                                 const double *d_albedo_mean, const RenderOptions &opt) {
    return run_denoise("denoise_albedo_mean_spatial", {.form = DenoiseForm::Means, .guides = DenoiseGuides::Albedo, .width = width, .height = height,
                                                       .first = d_mean, .second = d_m2, .count = samples, .albedo = d_albedo_mean, .spatial = true}, opt);
}

std::vector<uint8_t> denoise_guided_mean(int32_t width, int32_t height, const double *d_mean, const double *d_m2, int32_t samples,
                                         const double *d_albedo_mean, const double *d_edge_mean, const RenderOptions &opt) {
    return run_denoise("denoise_guided_mean", {.form = DenoiseForm::Means, .guides = DenoiseGuides::Edge, .width = width, .height = height,
                                               .first = d_mean, .second = d_m2, .count = samples, .albedo = d_albedo_mean, .edge = d_edge_mean,
                                               .spatial = opt.live_denoise_spatial > 0}, opt);
}

std::vector<uint8_t> denoise_guided_views(int32_t width, int32_t height, int32_t n_views, const double *d_sum, const double *d_sum_sq, int32_t spp,
                                          const double *d_albedo_sum, int32_t albedo_spp, const double *d_edge_sum, int32_t edge_spp,
                                          const RenderOptions &opt) {
    return run_denoise("denoise_guided_views", {.form = DenoiseForm::Views, .guides = DenoiseGuides::Edge, .width = width, .height = height,
                                                .first = d_sum, .second = d_sum_sq, .count = spp, .albedo = d_albedo_sum, .albedo_count = albedo_spp,
                                                .edge = d_edge_sum, .edge_count = edge_spp, .n_views = n_views}, opt);
}

// The albedo frame of a render (opt.denoise_albedo): the albedo scene of `desc` on device 0, rendered over the samples [0, spp) of
// every pixel with the render's seed under `cam` with a white background, into a new device frame of sums (the caller frees it).
// `surface_ids` (opt.denoise_edges): the surface-ID scene under `cam` with a black background instead.  `means` (the live route's edge
// guide): the frame of running means rt_render_mean_device gives over those samples, not their sums.
static int render_albedo_sums(const rt_scene_desc &desc, const rt_camera &cam, uint64_t seed, int32_t spp, void **d_albedo, bool surface_ids = false,
                              bool means = false) {
    rt_scene *scene = nullptr;
    int rc = surface_ids ? rt_scene_create_surface_ids(&desc, 0, nullptr, &scene) : rt_scene_create_albedo(&desc, 0, nullptr, &scene);
    if (rc == RT_OK) rc = rt_device_malloc(0, (int64_t)cam.image_width * cam.image_height * 3 * (int64_t)sizeof(double), d_albedo);
    if (rc == RT_OK) {
        rt_camera white = cam;
        white.background = surface_ids ? rt_vec3{0.0, 0.0, 0.0} : rt_vec3{1.0, 1.0, 1.0};
        rt_render_params p{};
        p.seed = seed; p.sample_begin = 0; p.sample_end = spp; p.max_depth = cam.max_depth;
        p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
        rc = means ? rt_render_mean_device(scene, &white, &p, static_cast<double *>(*d_albedo), nullptr, nullptr)
                   : rt_render_device(scene, &white, &p, static_cast<double *>(*d_albedo), nullptr);
        // (the scene is destroyed below while the render may still run: wait for the frame first)
        double probe = 0.0;
        if (rc == RT_OK) rc = rt_device_download(0, &probe, *d_albedo, (int64_t)sizeof probe, nullptr);
    }
    rt_scene_destroy(scene);
    return rc;
}

// A render on device 0 that is traced small and shown large (opt.upsample): the beauty frame under rt_camera_scaled — its sums, or with
// opt.denoise its moments, filtered at the low size under low-size guides — the full-size guide frames asked for, the upsampler, and
// then bloom and the tone-mapping stage if they are on, or the plain output stage on the full-size means.  Everything stays on the
// device until the display bytes, or the means they are made from, come back.
static std::vector<uint8_t> render_upsampled_rgb8(const Camera &camera, const Hittable &world, const RenderOptions &opt) {
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const rt_camera cam = camera.pod();
    rt_camera low;
    if (rt_camera_scaled(&cam, opt.upsample, &low) != RT_OK) throw std::runtime_error(std::string("render: ") + rt_last_error());
    const int32_t w = cam.image_width, h = cam.image_height, lw = low.image_width, lh = low.image_height, spp = cam.samples_per_pixel;
    const int64_t frame = (int64_t)w * h * 3 * (int64_t)sizeof(double), low_frame = (int64_t)lw * lh * 3 * (int64_t)sizeof(double);
    rt_scene *scene = nullptr;
    void *d_sum = nullptr, *d_sq = nullptr, *d_low_alb = nullptr, *d_low_ids = nullptr, *d_low_mean = nullptr, *d_work = nullptr, *d_alb = nullptr,
         *d_ids = nullptr, *d_out = nullptr;
    auto cleanup = [&]() {
        for (void *p : {d_sum, d_sq, d_low_alb, d_low_ids, d_low_mean, d_work, d_alb, d_ids, d_out}) rt_device_free(0, p);
        rt_scene_destroy(scene);
    };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, low_frame, &d_sum));
    check(rt_device_malloc(0, frame, &d_out));
    rt_render_params p{};
    p.seed = opt.seed; p.sample_begin = 0; p.sample_end = spp; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    const double *d_low = static_cast<const double *>(d_sum);
    int32_t low_spp = spp;
    if (opt.denoise) { // the low frame's own filter, with its guides rendered under the scaled camera
        check(rt_device_malloc(0, low_frame, &d_sq));
        check(rt_device_malloc(0, low_frame, &d_low_mean));
        check(rt_render_moments_device(scene, &low, &p, static_cast<double *>(d_sum), static_cast<double *>(d_sq), nullptr));
        if (opt.denoise_albedo) check(render_albedo_sums(desc, low, opt.seed, spp, &d_low_alb));
        if (opt.denoise_edges) check(render_albedo_sums(desc, low, opt.seed, spp, &d_low_ids, true));
        const DenoiseRequest r{.form = DenoiseForm::Sums, .guides = opt.denoise_edges ? DenoiseGuides::Edge : opt.denoise_albedo ? DenoiseGuides::Albedo : DenoiseGuides::None,
                               .width = lw, .height = lh, .first = static_cast<const double *>(d_sum), .second = static_cast<const double *>(d_sq), .count = spp,
                               .albedo = static_cast<const double *>(d_low_alb), .albedo_count = spp, .edge = static_cast<const double *>(d_low_ids), .edge_count = spp};
        const int64_t work = denoise_workspace_bytes(r);
        if (work < 0) { cleanup(); throw std::runtime_error("render: no denoise workspace for a frame of this size"); }
        check(rt_device_malloc(0, work, &d_work));
        double *out = static_cast<double *>(d_low_mean);
        check(denoise_into(r, opt, out, nullptr, d_work));
        d_low = out;
        low_spp = 1; // the filter writes means
    } else {
        check(rt_render_device(scene, &low, &p, static_cast<double *>(d_sum), nullptr));
    }
    if (opt.upsample_albedo) check(render_albedo_sums(desc, cam, opt.seed, spp, &d_alb));
    if (opt.upsample_edges) check(render_albedo_sums(desc, cam, opt.seed, spp, &d_ids, true));
    std::vector<uint8_t> px;
    try {
        upsample_device(w, h, d_low, low_spp, static_cast<const double *>(d_alb), spp, static_cast<const double *>(d_ids), spp, static_cast<double *>(d_out), opt);
        compare_device(w, h, static_cast<const double *>(d_out), 1, nullptr, opt);
        if (tonemapped(opt)) {
            px = staged_device(w, h, static_cast<const double *>(d_out), 1, nullptr, false, opt);
        } else {
            std::vector<double> means((size_t)w * (size_t)h * 3u);
            if (rt_device_download(0, means.data(), d_out, frame, nullptr) != RT_OK) throw std::runtime_error(std::string("render: ") + rt_last_error());
            px = resolve_rgb8(means, 1);
        }
    } catch (...) { cleanup(); throw; }
    cleanup();
    return px;
}

// A plain render on device 0 that ends in the denoiser: the frame's sums and sums of squares (rt_render_moments_device) stay on the
// device, are filtered there, and only the display bytes come back.
static std::vector<uint8_t> render_denoised_rgb8(const Camera &camera, const Hittable &world, const RenderOptions &opt) {
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const rt_camera cam = camera.pod();
    const int64_t n_pix = (int64_t)cam.image_width * cam.image_height;
    rt_scene *scene = nullptr;
    void *d_sum = nullptr, *d_sq = nullptr, *d_alb = nullptr, *d_ids = nullptr; // (d_alb: only with opt.denoise_albedo; d_ids: with opt.denoise_edges)
    auto cleanup = [&]() { rt_device_free(0, d_sum); rt_device_free(0, d_sq); rt_device_free(0, d_alb); rt_device_free(0, d_ids); rt_scene_destroy(scene); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, n_pix * 3 * (int64_t)sizeof(double), &d_sum));
    check(rt_device_malloc(0, n_pix * 3 * (int64_t)sizeof(double), &d_sq));
    rt_render_params p{};
    p.seed = opt.seed; p.sample_begin = 0; p.sample_end = cam.samples_per_pixel; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    check(rt_render_moments_device(scene, &cam, &p, static_cast<double *>(d_sum), static_cast<double *>(d_sq), nullptr));
    if (opt.denoise_albedo) check(render_albedo_sums(desc, cam, opt.seed, cam.samples_per_pixel, &d_alb));
    if (opt.denoise_edges) check(render_albedo_sums(desc, cam, opt.seed, cam.samples_per_pixel, &d_ids, true));
    std::vector<uint8_t> px;
    try {
        px = opt.denoise_edges
                 ? denoise_guided(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                                  cam.samples_per_pixel, nullptr, static_cast<const double *>(d_alb), cam.samples_per_pixel,
                                  static_cast<const double *>(d_ids), cam.samples_per_pixel, opt)
             : opt.denoise_albedo
                 ? denoise_albedo(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                                  cam.samples_per_pixel, nullptr, static_cast<const double *>(d_alb), cam.samples_per_pixel, opt)
                 : denoise(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                           cam.samples_per_pixel, nullptr, opt);
    } catch (...) { cleanup(); throw; }
    cleanup();
    return px;
}

void robust_device(int32_t width, int32_t height, int32_t blocks, const double *d_stack, int32_t spp, double *d_mean_out, double *d_m2_out,
                   const RenderOptions &opt) {
    rt_robust_params rp;
    if (rt_robust_params_init_sized(&rp, sizeof rp) != RT_OK) throw std::runtime_error(std::string("robust: ") + rt_last_error());
    rp.mode = opt.robust_mode; rp.trim = opt.robust_trim;
    if (opt.robust_gain > 0.0) rp.gain = opt.robust_gain;
    if (rt_robust_device(width, height, blocks, d_stack, spp, &rp, d_mean_out, d_m2_out, nullptr) != RT_OK)
        throw std::runtime_error(std::string("robust: ") + rt_last_error());
}

// A firefly-robust render on device 0 (opt.robust_blocks = K): K sub-frames of spp / K samples under the camera with seeds seed + k
// from one rt_render_views_device call, combined on the device by rt_robust_device; the frame of robust means goes through the
// means-form output — with opt.denoise, with its M2 and samples = K through rt_denoise_mean_device first — and only the bytes come back.
static std::vector<uint8_t> render_robust_rgb8(const Camera &camera, const Hittable &world, const RenderOptions &opt) {
    const rt_camera cam = camera.pod();
    const int32_t K = opt.robust_blocks, w = cam.image_width, h = cam.image_height;
    if (K < 1 || K > RT_ROBUST_MAX_BLOCKS) throw std::runtime_error("render: robust_blocks must be from 1 to 32");
    if (cam.samples_per_pixel % K != 0)
        throw std::runtime_error("render: robust_blocks = " + std::to_string(K) + " does not divide the " + std::to_string(cam.samples_per_pixel) +
                                 " samples per pixel: every block takes spp / robust_blocks of them");
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const int64_t n_pix = (int64_t)w * h, frame_bytes = n_pix * 3 * (int64_t)sizeof(double);
    rt_scene *scene = nullptr;
    void *d_stack = nullptr, *d_mean = nullptr, *d_m2 = nullptr, *d_rgba8 = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_stack); rt_device_free(0, d_mean); rt_device_free(0, d_m2); rt_device_free(0, d_rgba8); rt_scene_destroy(scene); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    std::vector<rt_view> views((size_t)K);
    for (int32_t k = 0; k < K; ++k) { views[(size_t)k].camera = cam; views[(size_t)k].seed = opt.seed + (uint64_t)k; }
    rt_render_params p{};
    p.sample_begin = 0; p.sample_end = cam.samples_per_pixel / K; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, frame_bytes * K, &d_stack));
    check(rt_device_malloc(0, frame_bytes, &d_mean));
    if (opt.denoise) check(rt_device_malloc(0, frame_bytes, &d_m2));
    check(rt_render_views_device(scene, views.data(), K, &p, static_cast<double *>(d_stack), nullptr));
    std::vector<uint8_t> px;
    try {
        robust_device(w, h, K, static_cast<const double *>(d_stack), p.sample_end, static_cast<double *>(d_mean), static_cast<double *>(d_m2), opt);
        if (!opt.denoise) compare_device(w, h, static_cast<const double *>(d_mean), 1, nullptr, opt); // (filtered: behind the filter, in denoise_mean)
        if (opt.denoise) px = denoise_mean(w, h, static_cast<const double *>(d_mean), static_cast<const double *>(d_m2), K, opt);
        else if (tonemapped(opt)) px = staged_device(w, h, static_cast<const double *>(d_mean), 1, nullptr, false, opt);
    } catch (...) { cleanup(); throw; }
    if (px.empty()) {
        check(rt_device_malloc(0, n_pix * 4, &d_rgba8));
        check(rt_resolve_rgba8_device(w, h, static_cast<const double *>(d_mean), static_cast<uint8_t *>(d_rgba8), nullptr));
        std::vector<uint8_t> rgba((size_t)n_pix * 4u);
        check(rt_device_download(0, rgba.data(), d_rgba8, n_pix * 4, nullptr));
        px.resize((size_t)n_pix * 3u);
        for (size_t q = 0; q < (size_t)n_pix; ++q) { px[3 * q] = rgba[4 * q]; px[3 * q + 1] = rgba[4 * q + 1]; px[3 * q + 2] = rgba[4 * q + 2]; }
    }
    cleanup();
    return px;
}

void panorama_device(int32_t width, int32_t height, const double *d_faces, int32_t face_size, int32_t guard, int32_t spp, double *d_mean_out) {
    if (width < 1 || height < 1 || (int64_t)width * height >= ((int64_t)1 << 27)) throw std::runtime_error("panorama: no frame of this size");
    std::vector<double> tables(2u * (size_t)width + 2u * (size_t)height);
    if (rt_panorama_tables(width, height, tables.data()) != RT_OK) throw std::runtime_error(std::string("panorama: ") + rt_last_error());
    const int64_t bytes = (int64_t)(tables.size() * sizeof(double));
    void *d_tables = nullptr;
    int rc = rt_device_malloc(0, bytes, &d_tables);
    if (rc == RT_OK) rc = rt_device_upload(0, d_tables, tables.data(), bytes, nullptr);
    if (rc == RT_OK) rc = rt_panorama_device(width, height, static_cast<const double *>(d_tables), d_faces, face_size, guard, spp, d_mean_out, nullptr);
    double done = 0.0; // (waits for the launch: the tables are freed behind it)
    if (rc == RT_OK) rc = rt_device_download(0, &done, d_mean_out, (int64_t)sizeof done, nullptr);
    const std::string msg = rc == RT_OK ? "" : rt_last_error();
    rt_device_free(0, d_tables);
    if (rc != RT_OK) throw std::runtime_error("panorama: " + msg);
}

// A panorama on device 0 (opt.panorama_width = W): the six cube-face views about the point from one rt_render_views_device call,
// resampled on the device by rt_panorama_device; the W x W / 2 frame of means goes through the means-form output and only the bytes
// come back.
static std::vector<uint8_t> render_panorama_rgb8(const Camera &camera, const Hittable &world, const RenderOptions &opt, int32_t &w, int32_t &h) {
    const rt_camera cam = camera.pod();
    w = opt.panorama_width; h = w / 2;
    if (w < 2 || w % 2 != 0 || w > 32768) throw std::runtime_error("render: panorama_width must be an even number from 2 to 32768");
    const int32_t g = opt.panorama_guard, F = opt.panorama_face > 0 ? opt.panorama_face : w / 4 + 2 * g;
    rt_camera faces[6];
    if (rt_camera_cube_faces(&cam, opt.panorama_at_given ? opt.panorama_at : nullptr, F, g, faces) != RT_OK)
        throw std::runtime_error(std::string("render: ") + rt_last_error());
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const int64_t n_pix = (int64_t)w * h, frame_bytes = n_pix * 3 * (int64_t)sizeof(double), face_bytes = (int64_t)F * F * 3 * (int64_t)sizeof(double);
    rt_scene *scene = nullptr;
    void *d_faces = nullptr, *d_mean = nullptr, *d_rgba8 = nullptr;
    auto cleanup = [&]() { rt_device_free(0, d_faces); rt_device_free(0, d_mean); rt_device_free(0, d_rgba8); rt_scene_destroy(scene); };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    std::vector<rt_view> views(6);
    for (int f = 0; f < 6; ++f) { views[(size_t)f].camera = faces[f]; views[(size_t)f].seed = opt.seed + (uint64_t)f; }
    rt_render_params p{};
    p.sample_begin = 0; p.sample_end = cam.samples_per_pixel; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, face_bytes * 6, &d_faces));
    check(rt_device_malloc(0, frame_bytes, &d_mean));
    check(rt_render_views_device(scene, views.data(), 6, &p, static_cast<double *>(d_faces), nullptr));
    std::vector<uint8_t> px;
    try {
        panorama_device(w, h, static_cast<const double *>(d_faces), F, g, p.sample_end, static_cast<double *>(d_mean));
        compare_device(w, h, static_cast<const double *>(d_mean), 1, nullptr, opt);
        if (tonemapped(opt)) px = staged_device(w, h, static_cast<const double *>(d_mean), 1, nullptr, false, opt);
    } catch (...) { cleanup(); throw; }
    if (px.empty()) {
        check(rt_device_malloc(0, n_pix * 4, &d_rgba8));
        check(rt_resolve_rgba8_device(w, h, static_cast<const double *>(d_mean), static_cast<uint8_t *>(d_rgba8), nullptr));
        std::vector<uint8_t> rgba((size_t)n_pix * 4u);
        check(rt_device_download(0, rgba.data(), d_rgba8, n_pix * 4, nullptr));
        px.resize((size_t)n_pix * 3u);
        for (size_t q = 0; q < (size_t)n_pix; ++q) { px[3 * q] = rgba[4 * q]; px[3 * q + 1] = rgba[4 * q + 1]; px[3 * q + 2] = rgba[4 * q + 2]; }
    }
    cleanup();
    return px;
}

// Adaptive sampling on device 0: the frame's sums and per-pixel spp stay on the device, are resolved there with each pixel's own
// spp, and only the bytes come back.
static std::vector<uint8_t> render_adaptive_rgb8(const Camera &camera, const Hittable &world, const RenderOptions &opt) {
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const rt_camera cam = camera.pod();
    const int64_t n_pix = (int64_t)cam.image_width * cam.image_height;
    rt_scene *scene = nullptr;
    void *d_sum = nullptr, *d_spp = nullptr, *d_rgb8 = nullptr, *d_sq = nullptr, *d_alb = nullptr, *d_ids = nullptr; // (d_sq: only with opt.denoise; d_alb: with opt.denoise_albedo; d_ids: with opt.denoise_edges)
    auto cleanup = [&]() {
        rt_device_free(0, d_sum); rt_device_free(0, d_spp); rt_device_free(0, d_rgb8); rt_device_free(0, d_sq); rt_device_free(0, d_alb); rt_device_free(0, d_ids);
        rt_scene_destroy(scene);
    };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, n_pix * 3 * (int64_t)sizeof(double), &d_sum));
    check(rt_device_malloc(0, n_pix * (int64_t)sizeof(int32_t), &d_spp));
    check(rt_device_malloc(0, n_pix * 3, &d_rgb8));
    rt_render_params p{};
    p.seed = opt.seed; p.sample_begin = 0; p.sample_end = cam.samples_per_pixel; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    rt_adaptive_params a;
    check(rt_adaptive_params_init_sized(&a, sizeof a));
    a.min_spp = opt.min_spp; a.batch_spp = opt.batch_spp; a.rel_threshold = opt.adaptive_rel; a.abs_threshold = opt.adaptive_abs;
    rt_adaptive_result res{};
    if (opt.denoise) check(rt_device_malloc(0, n_pix * 3 * (int64_t)sizeof(double), &d_sq));
    check(rt_render_adaptive_device(scene, &cam, &p, &a, static_cast<double *>(d_sum), static_cast<int32_t *>(d_spp), static_cast<double *>(d_sq), nullptr, &res));
    std::vector<uint8_t> px((size_t)n_pix * 3u);
    std::vector<int32_t> spp((size_t)n_pix);
    if (opt.denoise) { // the frame is written from the denoised mean: every pixel's own spp is its n (the albedo frame: the maximum's)
        if (opt.denoise_albedo) check(render_albedo_sums(desc, cam, opt.seed, cam.samples_per_pixel, &d_alb));
        if (opt.denoise_edges) check(render_albedo_sums(desc, cam, opt.seed, cam.samples_per_pixel, &d_ids, true)); // (the maximum spp, as the albedo frame)
        try {
            px = opt.denoise_edges
                     ? denoise_guided(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq), 0,
                                      static_cast<const int32_t *>(d_spp), static_cast<const double *>(d_alb), cam.samples_per_pixel,
                                      static_cast<const double *>(d_ids), cam.samples_per_pixel, opt)
                 : opt.denoise_albedo
                     ? denoise_albedo(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq), 0,
                                      static_cast<const int32_t *>(d_spp), static_cast<const double *>(d_alb), cam.samples_per_pixel, opt)
                     : denoise(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq), 0,
                               static_cast<const int32_t *>(d_spp), opt);
        } catch (...) { cleanup(); throw; }
    } else if (tonemapped(opt)) { // each pixel's own spp is its n, through the map
        try { compare_device(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), 1, static_cast<const int32_t *>(d_spp), opt); }
        catch (...) { cleanup(); throw; }
        try { px = staged_device(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), 1, static_cast<const int32_t *>(d_spp), false, opt); }
        catch (...) { cleanup(); throw; }
    } else {
        try { compare_device(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), 1, static_cast<const int32_t *>(d_spp), opt); }
        catch (...) { cleanup(); throw; }
        check(rt_resolve_rgb8_spp_device(cam.image_width, cam.image_height, static_cast<const double *>(d_sum), static_cast<const int32_t *>(d_spp),
                                         static_cast<uint8_t *>(d_rgb8), nullptr));
        check(rt_device_download(0, px.data(), d_rgb8, n_pix * 3, nullptr));
    }
    check(rt_device_download(0, spp.data(), d_spp, n_pix * (int64_t)sizeof(int32_t), nullptr));
    cleanup();
    int32_t lo = spp.empty() ? 0 : spp[0], hi = lo;
    for (int32_t v : spp) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    if (!opt.quiet)
        printf("Adaptive: mean %.2f spp, min %d, max %d, %d launches, %lld samples\n", n_pix ? (double)res.samples / (double)n_pix : 0.0, lo, hi,
               res.launches, (long long)res.samples);
    return px;
}

// the samples per pixel of the full-size guide frames a live session with opt.upsample renders once, before its first pass (fewer if
// the session itself settles on fewer): first-hit frames, whose only noise is the anti-aliasing of their edges
constexpr int32_t LIVE_UPSAMPLE_GUIDE_SPP = 16;

// The running mean and its display frame stay on the device; every pass is one rt_render_mean_device call (the render launches and one
// reduction that also writes the RGBA8 frame), and only the bytes to show come back.
std::vector<uint8_t> live_render(const Camera &camera, const Hittable &world, const RenderOptions &asked,
                                 const std::function<void(const std::vector<uint8_t> &, int)> &on_frame, std::vector<uint8_t> *final_film) {
    // every frame shown is RGBA8 whatever asked.format says: the passes run under `opt`, the options without the film format, and the
    // format shapes only *final_film, made from the last pass's means
    RenderOptions opt = asked;
    opt.format = FILM_PNG;
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    const rt_camera full = camera.pod();
    // opt.upsample: every pass traces and filters the frame of the scaled camera `cam`; the frame shown is rt_upsample_device's, at the
    // full size, under full-size guide frames rendered ONCE, before the first pass (d_up_alb, d_up_ids); they, the full-size frame d_full
    // and the upsampler's workspace are kept across the passes
    const bool upsampled = opt.upsample > 0;
    rt_camera cam = full;
    if (upsampled && rt_camera_scaled(&full, opt.upsample, &cam) != RT_OK) throw std::runtime_error(std::string("live_render: ") + rt_last_error());
    const int32_t fw = full.image_width, fh = full.image_height;
    const int64_t n_pix = (int64_t)cam.image_width * cam.image_height, n_shown = (int64_t)fw * fh; // traced and shown pixels
    std::vector<uint8_t> frame((size_t)n_shown * 4u, 0);
    for (size_t k = 3; k < frame.size(); k += 4) frame[k] = 0xff; // color_to_rgb(Color::ZERO), alpha 0xff
    const int last = cam.samples_per_pixel - 1; // `if num_samples < spp` (src/renderer.rs:104): divisors 1 .. spp - 1
    if (last <= 0) {
        if (final_film && filmed(asked)) *final_film = film_host(std::vector<double>((size_t)n_shown * 3u, 0.0), fw, fh, 1, asked);
        return frame;
    }
    const int pass = opt.live_spp > 0 ? opt.live_spp : 1;
    // opt.live_denoise: the pass keeps M2 beside the mean, and the frame shown is the filter's, written to d_shown and its bytes to
    // d_rgba8: the running frames (d_mean, d_m2, and the guided filter's running albedo mean d_alb) are the filter's inputs only
    // opt.live_denoise_edges: the surface-ID scene's frame of means d_ids, rendered ONCE, before the first pass, is every pass's edge guide
    const bool edges = opt.live_denoise_edges;
    const bool denoised = opt.live_denoise || opt.live_denoise_albedo || edges, guided = opt.live_denoise_albedo;
    if (opt.panorama_width != 0) throw std::runtime_error("live_render: panorama_width resamples the cube faces of one render() call: it cannot be combined with the live route");
    if (opt.robust_blocks != 0) throw std::runtime_error("live_render: robust_blocks combines the sub-frames of one render() call: it cannot be combined with the live route");
    if (compared(opt)) throw std::runtime_error("live_render: compare_file measures the one frame of a render() call: it cannot be combined with the live route");
    // opt.live_stop_noise >= 0: every pass keeps M2 (the moments route, whatever is shown), and the noise of (d_mean, d_m2) is reduced
    // behind it into d_noise, four doubles that lie 8-byte aligned BEHIND the display bytes in d_rgba8's allocation
    const bool stopping = opt.live_stop_noise >= 0.0;
    if (opt.live_stop_noise != opt.live_stop_noise) throw std::runtime_error("live_render: live_stop_noise must be a number");
    if (edges && opt.upsample > 0) throw std::runtime_error("live_render: live_denoise_edges cannot be combined with upsample (the guide would have to be made at the low size)");
    const int32_t w = cam.image_width, h = cam.image_height;
    rt_scene *scene = nullptr, *albedo_scene = nullptr;
    void *d_mean = nullptr, *d_rgba8 = nullptr, *d_m2 = nullptr, *d_alb = nullptr, *d_shown = nullptr, *d_work = nullptr;
    void *d_up_alb = nullptr, *d_up_ids = nullptr, *d_full = nullptr, *d_up_work = nullptr, *d_ids = nullptr, *d_noise_work = nullptr;
    auto cleanup = [&]() {
        rt_device_free(0, d_noise_work); rt_device_free(0, d_ids); rt_device_free(0, d_mean); rt_device_free(0, d_rgba8); rt_device_free(0, d_m2); rt_device_free(0, d_alb); rt_device_free(0, d_shown);
        rt_device_free(0, d_work); rt_device_free(0, d_up_alb); rt_device_free(0, d_up_ids); rt_device_free(0, d_full); rt_device_free(0, d_up_work);
        rt_scene_destroy(scene); rt_scene_destroy(albedo_scene);
    };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("live_render: " + msg); } };
    const int64_t frame_bytes = n_pix * 3 * (int64_t)sizeof(double);
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, frame_bytes, &d_mean));
    const int64_t shown_bytes = n_shown * 4, noise_at = (shown_bytes + 7) / 8 * 8; // the four doubles' place behind the bytes
    check(rt_device_malloc(0, stopping ? noise_at + 4 * (int64_t)sizeof(double) : shown_bytes, &d_rgba8));
    double *const d_noise = stopping ? reinterpret_cast<double *>(static_cast<uint8_t *>(d_rgba8) + noise_at) : nullptr;
    std::vector<uint8_t> handed; // the pass's one download where the bytes and the doubles come back together
    rt_frame_noise_params noise_params;
    if (stopping) {
        const int64_t noise_work = rt_metrics_workspace_bytes(w, h);
        if (noise_work < 0) { cleanup(); throw std::runtime_error("live_render: no metrics workspace for a frame of this size"); }
        check(rt_frame_noise_params_init_sized(&noise_params, sizeof noise_params));
        check(rt_device_malloc(0, noise_work, &d_noise_work));
        if (!denoised) check(rt_device_malloc(0, frame_bytes, &d_m2));
        handed.resize((size_t)noise_at + 4u * sizeof(double));
    }
    rt_upsample_params up{};
    const int32_t guide_spp = last < LIVE_UPSAMPLE_GUIDE_SPP ? last : LIVE_UPSAMPLE_GUIDE_SPP;
    if (upsampled) {
        try { up = upsample_params(opt); } catch (...) { cleanup(); throw; }
        const int64_t up_work = rt_upsample_workspace_bytes(fw, fh, up.factor);
        if (up_work < 0) { cleanup(); throw std::runtime_error("live_render: no upsample workspace for a frame of this size at this factor"); }
        check(rt_device_malloc(0, n_shown * 3 * (int64_t)sizeof(double), &d_full));
        check(rt_device_malloc(0, up_work, &d_up_work));
        if (opt.upsample_albedo) check(render_albedo_sums(desc, full, opt.seed, guide_spp, &d_up_alb));
        if (opt.upsample_edges) check(render_albedo_sums(desc, full, opt.seed, guide_spp, &d_up_ids, true));
    }
    rt_camera white = cam;
    white.background = rt_vec3{1.0, 1.0, 1.0};
    // every pass's filter; opt.live_denoise_spatial > 0: through the spatial entry points, so that the first pass is filtered too
    DenoiseRequest filter{.form = DenoiseForm::Means, .guides = edges ? DenoiseGuides::Edge : guided ? DenoiseGuides::Albedo : DenoiseGuides::None,
                          .width = w, .height = h, .first = nullptr, .second = nullptr, .count = 0, .spatial = opt.live_denoise_spatial > 0};
    if (denoised) {
        if (guided) {
            check(rt_scene_create_albedo(&desc, 0, nullptr, &albedo_scene));
            check(rt_device_malloc(0, frame_bytes, &d_alb));
        }
        filter.albedo = static_cast<const double *>(d_alb); // (null without the albedo guide: the plain filter with the edge guide)
        const int64_t work = denoise_workspace_bytes(filter);
        if (work < 0) { cleanup(); throw std::runtime_error("live_render: no denoise workspace for a frame of this size"); }
        check(rt_device_malloc(0, frame_bytes, &d_m2));
        check(rt_device_malloc(0, frame_bytes, &d_shown));
        check(rt_device_malloc(0, work, &d_work));
        if (edges) check(render_albedo_sums(desc, cam, opt.seed, guide_spp, &d_ids, true, true));
        filter.first = static_cast<const double *>(d_mean); filter.second = static_cast<const double *>(d_m2); filter.edge = static_cast<const double *>(d_ids);
    }
    // with the tone-mapping stage on, the pass and the filters write no bytes (a null d_rgba8): the stage makes the frame shown from
    // the running mean — or, filtered, from d_shown — and the mean itself is never touched
    // ... and with the upsampler on it is the upsampler that writes the bytes, at the full size
    uint8_t *const d_bytes = tonemapped(opt) || upsampled ? nullptr : static_cast<uint8_t *>(d_rgba8);
    for (int begin = 0; begin < last; begin += pass) {
        const int end = begin + pass < last ? begin + pass : last;
        rt_render_params p{};
        p.seed = opt.seed; p.sample_begin = begin; p.sample_end = end; p.max_depth = cam.max_depth;
        p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
        if (!denoised && stopping) { // the moments route: the same mean and the same bytes, with M2 beside them
            check(rt_render_mean_moments_device(scene, &cam, &p, static_cast<double *>(d_mean), static_cast<double *>(d_m2), d_bytes, nullptr));
        } else if (!denoised) {
            check(rt_render_mean_device(scene, &cam, &p, static_cast<double *>(d_mean), d_bytes, nullptr));
        } else {
            check(rt_render_mean_moments_device(scene, &cam, &p, static_cast<double *>(d_mean), static_cast<double *>(d_m2), nullptr, nullptr));
            if (guided) check(rt_render_mean_device(albedo_scene, &white, &p, static_cast<double *>(d_alb), nullptr, nullptr));
            filter.count = end;
            check(denoise_into(filter, opt, static_cast<double *>(d_shown), d_bytes, d_work));
        }
        const double *d_means = static_cast<const double *>(denoised ? d_shown : d_mean); // the pass's frame of means, at the traced size
        if (upsampled) {
            check(rt_upsample_device(fw, fh, d_means, 1, static_cast<const double *>(d_up_alb), guide_spp, static_cast<const double *>(d_up_ids), guide_spp,
                                     &up, static_cast<double *>(d_full), tonemapped(opt) ? nullptr : static_cast<uint8_t *>(d_rgba8), d_up_work, nullptr));
            d_means = static_cast<const double *>(d_full);
        }
        // the noise of the running frames, enqueued in front of the frame's hand-off: that hand-off's wait covers it
        if (stopping)
            check(rt_frame_noise_device(w, h, RT_METRICS_MEANS, static_cast<const double *>(d_mean), static_cast<const double *>(d_m2), end, nullptr, &noise_params,
                                        d_noise, d_noise_work, nullptr));
        double noise4[4] = {0.0, 0.0, 0.0, 0.0};
        if (tonemapped(opt)) {
            try { frame = staged_device(fw, fh, d_means, 1, nullptr, true, opt); }
            catch (...) { cleanup(); throw; }
            // (the stage has its own output buffer and has waited for the stream: the doubles are ready, this copy waits for nothing)
            if (stopping) check(rt_device_download(0, noise4, d_noise, (int64_t)sizeof noise4, nullptr));
        } else if (stopping) { // one download: the bytes, and the four doubles behind them
            check(rt_device_download(0, handed.data(), d_rgba8, (int64_t)handed.size(), nullptr));
            memcpy(frame.data(), handed.data(), (size_t)shown_bytes);
            memcpy(noise4, handed.data() + noise_at, sizeof noise4);
        } else {
            check(rt_device_download(0, frame.data(), d_rgba8, n_shown * 4, nullptr));
        }
        if (on_frame) {
            try { on_frame(frame, end); } catch (...) { cleanup(); throw; }
        }
        bool stopped = false;
        if (stopping) {
            if (!opt.quiet) printf("live-stop-pass: samples=%d noise=%.17g\n", end, noise4[2]);
            stopped = end >= opt.live_stop_min_samples && noise4[2] <= opt.live_stop_noise;
            if (stopped || end == last) printf("live-stop: samples=%d noise=%.17g\n", end, noise4[2]);
        }
        if ((end == last || stopped) && final_film && filmed(asked)) { // the frame just shown, in the film format: bloom and the stage on the same means
            try { *final_film = staged_device(fw, fh, d_means, 1, nullptr, false, asked); }
            catch (...) { cleanup(); throw; }
        }
        if (stopped) break;
    }
    cleanup();
    return frame;
}

// An orbit on device 0 that ends in the denoiser (opt.orbit_denoise, opt.orbit_denoise_albedo, opt.orbit_denoise_edges): every view's sums and sums of squares
// from one rt_render_views_moments_device call stay on the device and are filtered there as one stack (rt_denoise_views_device); the
// guided form takes its albedo frames from one rt_render_views_device over the albedo scene, under the views' cameras with a white
// background and their seeds.  Returns the views' RGB bytes, one frame behind the other.
static std::vector<uint8_t> render_orbit_denoised_rgb8(const rt_scene_desc &desc, const std::vector<rt_view> &views, const rt_render_params &p,
                                                       const RenderOptions &opt) {
    const rt_camera &cam = views[0].camera;
    const int32_t n = (int32_t)views.size();
    const int64_t bytes = (int64_t)n * cam.image_width * cam.image_height * 3 * (int64_t)sizeof(double);
    rt_scene *scene = nullptr, *albedo = nullptr, *ids = nullptr;
    void *d_sum = nullptr, *d_sq = nullptr, *d_alb = nullptr, *d_ids = nullptr; // (d_alb: only with opt.orbit_denoise_albedo; d_ids: with opt.orbit_denoise_edges)
    auto cleanup = [&]() {
        rt_device_free(0, d_sum); rt_device_free(0, d_sq); rt_device_free(0, d_alb); rt_device_free(0, d_ids);
        rt_scene_destroy(scene); rt_scene_destroy(albedo); rt_scene_destroy(ids);
    };
    auto check = [&](int rc) { if (rc != RT_OK) { const std::string msg = rt_last_error(); cleanup(); throw std::runtime_error("render: " + msg); } };
    check(rt_scene_create(&desc, 0, &scene));
    check(rt_device_malloc(0, bytes, &d_sum));
    check(rt_device_malloc(0, bytes, &d_sq));
    check(rt_render_views_moments_device(scene, views.data(), n, &p, static_cast<double *>(d_sum), static_cast<double *>(d_sq), nullptr));
    if (opt.orbit_denoise_albedo) {
        std::vector<rt_view> white(views);
        for (rt_view &v : white) v.camera.background = rt_vec3{1.0, 1.0, 1.0};
        check(rt_scene_create_albedo(&desc, 0, nullptr, &albedo));
        check(rt_device_malloc(0, bytes, &d_alb));
        check(rt_render_views_device(albedo, white.data(), n, &p, static_cast<double *>(d_alb), nullptr));
    }
    if (opt.orbit_denoise_edges) { // every view's edge guide from one launch over the surface-ID scene, black-background cameras
        std::vector<rt_view> black(views);
        for (rt_view &v : black) v.camera.background = rt_vec3{0.0, 0.0, 0.0};
        check(rt_scene_create_surface_ids(&desc, 0, nullptr, &ids));
        check(rt_device_malloc(0, bytes, &d_ids));
        check(rt_render_views_device(ids, black.data(), n, &p, static_cast<double *>(d_ids), nullptr));
    }
    std::vector<uint8_t> px;
    try { // (the filter's download waits for everything enqueued before it: the scenes are destroyed after it)
        px = opt.orbit_denoise_edges
                 ? denoise_guided_views(cam.image_width, cam.image_height, n, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                                        cam.samples_per_pixel, static_cast<const double *>(d_alb), cam.samples_per_pixel,
                                        static_cast<const double *>(d_ids), cam.samples_per_pixel, opt)
             : opt.orbit_denoise_albedo
                 ? denoise_albedo_views(cam.image_width, cam.image_height, n, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                                        cam.samples_per_pixel, static_cast<const double *>(d_alb), cam.samples_per_pixel, opt)
                 : denoise_views(cam.image_width, cam.image_height, n, static_cast<const double *>(d_sum), static_cast<const double *>(d_sq),
                                 cam.samples_per_pixel, opt);
    } catch (...) { cleanup(); throw; }
    cleanup();
    return px;
}

// An orbit on device 0: every view's frame in one rt_render_views call, one PNG per view.
static void render_orbit(const Camera &camera, const Hittable &world, const std::string &output_file_name, const RenderOptions &opt) {
    using clock = std::chrono::steady_clock;
    auto now = clock::now();
    SceneDescriber sd;
    const rt_ref root = world.describe(sd);
    const rt_scene_desc desc = sd.desc(root);
    std::vector<rt_view> views((size_t)opt.orbit);
    for (int k = 0; k < opt.orbit; ++k) {
        CameraSettings s = camera.settings;
        s.look_from = orbit_look_from(camera.settings.look_from, camera.settings.look_at, camera.settings.vup, k, opt.orbit);
        views[(size_t)k].camera = Camera(s).pod();
        views[(size_t)k].seed = opt.seed + (uint64_t)k;
    }
    const rt_camera &cam = views[0].camera;
    const size_t frame = (size_t)cam.image_width * (size_t)cam.image_height * 3u;
    rt_scene *scene = nullptr;
    rt_render_params p{};
    p.sample_begin = 0; p.sample_end = cam.samples_per_pixel; p.max_depth = cam.max_depth;
    p.shard_count = 1; p.out_layout = RT_OUT_FRAME;
    if (opt.orbit_denoise || opt.orbit_denoise_albedo || opt.orbit_denoise_edges) {
        const std::vector<uint8_t> px = render_orbit_denoised_rgb8(desc, views, p, opt);
        if (!opt.quiet) printf("Render time: %.2fs (%d views, denoised)\n", std::chrono::duration<double>(clock::now() - now).count(), opt.orbit);
        now = clock::now();
        const size_t one = px.size() / (size_t)opt.orbit; // a view's bytes, in the format asked for
        for (int k = 0; k < opt.orbit; ++k) {
            char suffix[16];
            snprintf(suffix, sizeof suffix, "_%03d", k);
            write_frame(output_file_name + suffix, cam.image_width, cam.image_height,
                        std::vector<uint8_t>(px.begin() + (ptrdiff_t)(one * (size_t)k), px.begin() + (ptrdiff_t)(one * (size_t)(k + 1))), opt);
        }
        if (!opt.quiet) printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
        return;
    }
    std::vector<double> sums(frame * views.size(), 0.0);
    int rc = rt_scene_create(&desc, 0, &scene);
    if (rc == RT_OK) rc = rt_render_views(scene, views.data(), opt.orbit, &p, sums.data());
    const std::string msg = rc == RT_OK ? "" : rt_last_error();
    rt_scene_destroy(scene);
    if (rc != RT_OK) throw std::runtime_error("render: " + msg);
    if (!opt.quiet) {
        const double render_s = std::chrono::duration<double>(clock::now() - now).count();
        printf("Render time: %.2fs (%d views, %.1f Msamples/s)\n", render_s, opt.orbit,
               (double)opt.orbit * (double)cam.image_width * (double)cam.image_height * (double)cam.samples_per_pixel / 1e6 / render_s);
    }
    now = clock::now();
    for (int k = 0; k < opt.orbit; ++k) {
        const std::vector<double> one(sums.begin() + (ptrdiff_t)(frame * (size_t)k), sums.begin() + (ptrdiff_t)(frame * (size_t)(k + 1)));
        char suffix[16];
        snprintf(suffix, sizeof suffix, "_%03d", k);
        const std::vector<uint8_t> px = tonemapped(opt) ? staged_rgb8(one, cam.image_width, cam.image_height, cam.samples_per_pixel, opt) // (each view its own frame)
                                                        : resolve_rgb8(one, cam.samples_per_pixel);
        write_frame(output_file_name + suffix, cam.image_width, cam.image_height, px, opt);
    }
    if (!opt.quiet) printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
}

void render(std::shared_ptr<Camera> camera, std::shared_ptr<Hittable> world, const std::string &output_file_name,
            const RenderOptions &opt) {
    using clock = std::chrono::steady_clock;
    auto now = clock::now();
    const int32_t w = (int32_t)camera->image_width, h = (int32_t)camera->image_height;
    if (opt.format < FILM_PNG || opt.format > FILM_PFM) throw std::runtime_error("render: format must be FILM_PNG, FILM_PNG16, FILM_HDR or FILM_PFM");
    if (filmed(opt) && (opt.gpus > 1 || opt.progressive_spp > 0))
        throw std::runtime_error("render: a format other than png is written by the film stage of a one-GPU, one-pass route: it cannot be combined with "
                                 "gpus > 1 or progressive_spp (the gather and the passes carry 8-bit frames)");
    if (compared(opt) && (opt.orbit > 0 || opt.gpus > 1 || opt.progressive_spp > 0))
        throw std::runtime_error("render: compare_file measures the one frame of a one-GPU, one-pass route: it cannot be combined with orbit, gpus > 1 or "
                                 "progressive_spp");
    if (compared(opt) && !(opt.compare_eps >= 0.0 && opt.compare_eps < 1e300)) throw std::runtime_error("render: compare_eps must be a finite number >= 0 (0: the default)");
    if (opt.upsample != 0 && (opt.upsample < 2 || opt.upsample > 4)) throw std::runtime_error("render: upsample must be 0 (off), 2, 3 or 4");
    if (opt.upsample > 0 && (opt.orbit > 0 || opt.adaptive || opt.gpus > 1 || opt.progressive_spp > 0))
        throw std::runtime_error("render: upsample is a one-GPU, one-pass route: it cannot be combined with orbit, adaptive, gpus > 1 or progressive_spp");
    if ((opt.upsample_albedo || opt.upsample_edges) && opt.upsample == 0) throw std::runtime_error("render: upsample_albedo and upsample_edges need upsample");
    if (opt.panorama_width != 0) {
        if (opt.adaptive || opt.orbit > 0 || opt.progressive_spp > 0 || opt.upsample > 0 || opt.robust_blocks != 0 || opt.denoise || opt.gpus > 1)
            throw std::runtime_error("render: panorama_width is a one-GPU, one-pass route of its own: it cannot be combined with adaptive, orbit, "
                                     "progressive_spp, upsample, robust_blocks, denoise or gpus > 1");
        int32_t pw = 0, ph = 0;
        const std::vector<uint8_t> px = render_panorama_rgb8(*camera, *world, opt, pw, ph);
        if (!opt.quiet) printf("Render time: %.2fs (panorama %d x %d)\n", std::chrono::duration<double>(clock::now() - now).count(), pw, ph);
        now = clock::now();
        write_frame(output_file_name, pw, ph, px, opt);
        if (!opt.quiet) printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
        return;
    }
    if (opt.robust_blocks != 0) {
        if (opt.adaptive || opt.orbit > 0 || opt.progressive_spp > 0 || opt.upsample > 0 || opt.gpus > 1)
            throw std::runtime_error("render: robust_blocks is a one-GPU, one-pass route of its own: it cannot be combined with adaptive, orbit, "
                                     "progressive_spp, upsample or gpus > 1");
        if (opt.denoise_albedo || opt.denoise_edges)
            throw std::runtime_error("render: robust_blocks filters its frame with the plain means form: it cannot be combined with denoise_albedo or denoise_edges");
        const std::vector<uint8_t> px = render_robust_rgb8(*camera, *world, opt);
        if (!opt.quiet) printf("Render time: %.2fs (%d robust blocks)\n", std::chrono::duration<double>(clock::now() - now).count(), opt.robust_blocks);
        now = clock::now();
        write_frame(output_file_name, w, h, px, opt);
        if (!opt.quiet) printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
        return;
    }
    if (opt.orbit > 0) {
        render_orbit(*camera, *world, output_file_name, opt);
        return;
    }
    if (opt.adaptive || opt.denoise || opt.upsample > 0) {
        const std::vector<uint8_t> px = opt.upsample > 0 ? render_upsampled_rgb8(*camera, *world, opt)
                                        : opt.adaptive   ? render_adaptive_rgb8(*camera, *world, opt)
                                                         : render_denoised_rgb8(*camera, *world, opt);
        if (!opt.quiet) printf("Render time: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
        now = clock::now();
        write_frame(output_file_name, w, h, px, opt);
        if (!opt.quiet) printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
        return;
    }
    // progressive passes: the PNG on disk always shows the mean of the samples traced so far
    auto on_pass = [&](const std::vector<double> &partial, int done) {
        if (opt.progressive_spp <= 0 || done >= camera->samples_per_pixel) return;
        write_png_rgb8(output_file_name + ".png", w, h, resolve_rgb8(partial, done).data());
        if (!opt.quiet) printf("  %d / %d spp\n", done, camera->samples_per_pixel);
    };
    const std::vector<double> sums = render_sums(*camera, *world, opt, on_pass);
    const double render_s = std::chrono::duration<double>(clock::now() - now).count();
    if (!opt.quiet) {
        const double msamples = (double)camera->image_width * (double)camera->image_height *
                                (double)camera->samples_per_pixel / 1e6;
        printf("Render time: %.2fs (%.1f Msamples/s)\n", render_s, msamples / render_s);
    }

    now = clock::now();
    compare_host(sums, w, h, camera->samples_per_pixel, opt);
    const std::vector<uint8_t> px = tonemapped(opt) ? staged_rgb8(sums, w, h, camera->samples_per_pixel, opt) : resolve_rgb8(sums, camera->samples_per_pixel);
    write_frame(output_file_name, w, h, px, opt);
    if (!opt.quiet)
        printf("PNG encoding: %.2fs\n", std::chrono::duration<double>(clock::now() - now).count());
}

} // namespace rt
