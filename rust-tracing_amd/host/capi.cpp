// C entry points of librt_host.so (include/rt_host.h).
#include "rt_host.h"
#include "color.hpp"
#include "image_io.hpp"
#include "renderer.hpp"
#include "scenes.hpp"
#include "../csrc/rt_tonemap_shared.h"
#include "../csrc/rt_bloom_shared.h"
#include "../csrc/rt_robust_shared.h"
#include "../csrc/rt_upsample_shared.h"
#include "../csrc/rt_panorama_shared.h"
#include "../csrc/rt_metrics_shared.h"
#include <cstring>
#include <exception>
#include <string>
#include <vector>

using namespace rt;

struct rth_scene {
    HittableList world;             // the list main hands to BVHNode::new (kept alive: the BVH shares its objects)
    std::shared_ptr<BVHNode> bvh;
    std::unique_ptr<Camera> camera;
    SceneDescriber sd;
    rt_scene_desc desc;
    rt_camera cam;
};

static thread_local std::string g_error;
static int fail(const std::string &msg) {
    g_error = msg;
    return -1;
}

extern "C" {

const char *rth_last_error(void) { return g_error.c_str(); }

int rth_scene_build(const rth_scene_options *options, rth_scene **out_scene) {
    if (!options || !out_scene) return fail("rth_scene_build: null argument");
    *out_scene = nullptr;
    try {
        SceneOptions so;
        so.image_width = options->image_width;
        so.aspect_ratio = options->aspect_ratio;
        so.samples_per_pixel = options->samples_per_pixel;
        so.max_depth = options->max_depth;
        so.earth_image = options->earth_image ? options->earth_image : "synthetic:1024x512";

        // (the policy is this thread's and is put back afterwards: the caller's later builds see what they saw before)
        struct PolicyScope {
            BvhPolicy saved = bvh_policy();
            ~PolicyScope() { bvh_policy() = saved; }
        } policy_scope;
        bvh_policy() = options->bvh_policy == 1 ? BvhPolicy::Sah : BvhPolicy::Reference;
        seed_rng(options->scene_seed);

        auto s = std::make_unique<rth_scene>();
        auto built = build_scene(options->scene, so);
        s->world = std::move(built.first);
        s->camera = std::make_unique<Camera>(built.second);
        s->bvh = std::make_shared<BVHNode>(s->world);
        const rt_ref root = s->bvh->describe(s->sd);
        s->desc = s->sd.desc(root);
        s->cam = s->camera->pod();
        *out_scene = s.release();
        return 0;
    } catch (const std::exception &e) {
        return fail(std::string("rth_scene_build: ") + e.what());
    }
}

void rth_scene_destroy(rth_scene *scene) { delete scene; }
const rt_scene_desc *rth_scene_desc(const rth_scene *scene) { return scene ? &scene->desc : nullptr; }
const rt_camera *rth_scene_camera(const rth_scene *scene) { return scene ? &scene->cam : nullptr; }

int rth_scene_camera_look(const rth_scene *scene, const double look_from[3], const double look_at[3], rt_camera *out) {
    if (!scene || !out) return fail("rth_scene_camera_look: null argument");
    CameraSettings s = scene->camera->settings;
    if (look_from) s.look_from = Point3(look_from[0], look_from[1], look_from[2]);
    if (look_at) s.look_at = Point3(look_at[0], look_at[1], look_at[2]);
    *out = Camera(s).pod();
    return 0;
}

int rth_scene_look(const rth_scene *scene, double look_from[3], double look_at[3], double vup[3]) {
    if (!scene) return fail("rth_scene_look: null argument");
    const CameraSettings &s = scene->camera->settings;
    if (look_from) { look_from[0] = s.look_from.x; look_from[1] = s.look_from.y; look_from[2] = s.look_from.z; }
    if (look_at) { look_at[0] = s.look_at.x; look_at[1] = s.look_at.y; look_at[2] = s.look_at.z; }
    if (vup) { vup[0] = s.vup.x; vup[1] = s.vup.y; vup[2] = s.vup.z; }
    return 0;
}

int rth_scene_orbit_look_from(const rth_scene *scene, int32_t k, int32_t n, double out_look_from[3]) {
    if (!scene || !out_look_from) return fail("rth_scene_orbit_look_from: null argument");
    if (n < 1) return fail("rth_scene_orbit_look_from: n must be at least 1");
    const CameraSettings &s = scene->camera->settings;
    const Point3 p = orbit_look_from(s.look_from, s.look_at, s.vup, k, n);
    out_look_from[0] = p.x; out_look_from[1] = p.y; out_look_from[2] = p.z;
    return 0;
}

int rth_resolve_rgb8(int32_t width, int32_t height, int32_t spp, const double *rgb_sum, uint8_t *out_rgb8) {
    if (!rgb_sum || !out_rgb8 || width <= 0 || height <= 0 || spp <= 0) return fail("rth_resolve_rgb8: bad argument");
    const size_t n = (size_t)width * (size_t)height;
    const FP inv = 1.0 / (FP)spp;
    for (size_t i = 0; i < n; ++i) {
        const auto rgb = color_to_rgb(Color(rgb_sum[3 * i] * inv, rgb_sum[3 * i + 1] * inv, rgb_sum[3 * i + 2] * inv));
        out_rgb8[3 * i] = rgb[0]; out_rgb8[3 * i + 1] = rgb[1]; out_rgb8[3 * i + 2] = rgb[2];
    }
    return 0;
}

// ---- tone mapping: the host mirror of rt_tonemap_device (include/rt_amd.h "tone mapping") ----

namespace {
struct LogPartial { double t; uint32_t count; };

// the normative reduction: 256 entries per block (the last one padded with +0.0, count 0), each block by the tree
// `for stride = 128 .. 1: e[i] = e[i] + e[i + stride]`, the block results the next level's entries, until one is left
LogPartial reduce_log_terms(std::vector<LogPartial> entries) {
    for (;;) {
        const size_t blocks = (entries.size() + 255u) / 256u;
        std::vector<LogPartial> next(blocks);
        for (size_t b = 0; b < blocks; ++b) {
            LogPartial e[256];
            for (size_t i = 0; i < 256; ++i) e[i] = b * 256u + i < entries.size() ? entries[b * 256u + i] : LogPartial{0.0, 0u};
            for (size_t stride = 128; stride >= 1; stride >>= 1)
                for (size_t i = 0; i < stride; ++i) { e[i].t = e[i].t + e[i + stride].t; e[i].count += e[i + stride].count; }
            next[b] = e[0];
        }
        if (blocks == 1) return next[0];
        entries.swap(next);
    }
}

// out4 = log_mean, Lavg, (double)count, scale (auto_key == 0: 0) of a frame of n pixels
void log_average(size_t n, const double *values, int32_t spp, const int32_t *spp_map, double delta, double exposure, double auto_key, double out4[4]) {
    std::vector<LogPartial> terms(n);
    for (size_t p = 0; p < n; ++p) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[p] : spp);
        terms[p].t = rtm::rt_log_luminance_term(values[3 * p] * inv, values[3 * p + 1] * inv, values[3 * p + 2] * inv, delta, &terms[p].count);
    }
    const LogPartial total = reduce_log_terms(std::move(terms));
    rtm::rt_log_average_result(total.t, total.count, exposure, auto_key, out4);
}
} // namespace

int rth_log_average_luminance(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map, double delta,
                              double *out4) {
    const std::string w("rth_log_average_luminance");
    if (width <= 0 || height <= 0) return fail(w + ": width and height must be positive");
    if ((int64_t)width * height >= rttm::MAX_PIXELS) return fail(w + ": width x height must be below 2^27 pixels");
    if (!values) return fail(w + ": values is null");
    if (!out4) return fail(w + ": out4 is null");
    if (spp < 1) return fail(w + ": spp must be at least 1");
    if (!rttm::positive_finite(delta)) return fail(w + ": delta must be a finite number > 0");
    log_average((size_t)width * (size_t)height, values, spp, spp_map, delta, 1.0, 0.0, out4);
    return 0;
}

int rth_tonemap(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map, const rt_tonemap_params *params,
                uint8_t *out_rgb8, uint8_t *out_rgba8) {
    const std::string w("rth_tonemap");
    if (width <= 0 || height <= 0) return fail(w + ": width and height must be positive");
    if ((int64_t)width * height >= rttm::MAX_PIXELS) return fail(w + ": width x height must be below 2^27 pixels");
    if (!values) return fail(w + ": values is null");
    if (!out_rgb8 && !out_rgba8) return fail(w + ": out_rgb8 and out_rgba8 are both null");
    if (spp < 1) return fail(w + ": spp must be at least 1");
    rt_tonemap_params p;
    if (!rttm::resolve(params, p)) return fail(w + ": rt_tonemap_params.struct_size is not one this library knows");
    if (const char *bad = rttm::bad_field(p)) return fail(w + ": " + bad);
    const size_t n = (size_t)width * (size_t)height;
    double scale = p.exposure;
    if (p.auto_key > 0.0) {
        double out4[4];
        log_average(n, values, spp, spp_map, p.delta, p.exposure, p.auto_key, out4);
        scale = out4[3];
    }
    const double w2 = p.white * p.white;
    for (size_t i = 0; i < n; ++i) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[i] : spp);
        uint8_t rgb[3];
        for (size_t c = 0; c < 3; ++c) {
            const double m = values[3 * i + c] * inv;
            const double x = m * scale;
            rgb[c] = rtm::rt_quantise(rtm::rt_gamma_encode(rtm::rt_tonemap(p.op, x, w2)));
        }
        if (out_rgb8) { out_rgb8[3 * i] = rgb[0]; out_rgb8[3 * i + 1] = rgb[1]; out_rgb8[3 * i + 2] = rgb[2]; }
        if (out_rgba8) { out_rgba8[4 * i] = rgb[0]; out_rgba8[4 * i + 1] = rgb[1]; out_rgba8[4 * i + 2] = rgb[2]; out_rgba8[4 * i + 3] = 0xff; }
    }
    return 0;
}

// ---- film output: the host mirror of rt_film_device (include/rt_amd.h "film output") ----

int rth_film(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map, const rt_tonemap_params *tone,
             int32_t format, void *out) {
    const std::string w("rth_film");
    if (width <= 0 || height <= 0) return fail(w + ": width and height must be positive");
    if ((int64_t)width * height >= rttm::MAX_PIXELS) return fail(w + ": width x height must be below 2^27 pixels");
    if (!values) return fail(w + ": values is null");
    if (!out) return fail(w + ": out is null");
    if (spp < 1) return fail(w + ": spp must be at least 1");
    if (!rttm::film_pixel_bytes(format)) return fail(w + ": format must be RT_FILM_RGBE, RT_FILM_F32 or RT_FILM_RGB16 (0..2)");
    rt_tonemap_params p;
    if (!rttm::resolve(tone, p)) return fail(w + ": rt_tonemap_params.struct_size is not one this library knows");
    if (const char *bad = rttm::bad_field(p)) return fail(w + ": " + bad);
    const size_t n = (size_t)width * (size_t)height;
    double scale = p.exposure;
    if (p.auto_key > 0.0) {
        double out4[4];
        log_average(n, values, spp, spp_map, p.delta, p.exposure, p.auto_key, out4);
        scale = out4[3];
    }
    const double w2 = p.white * p.white;
    uint8_t *bytes = static_cast<uint8_t *>(out); // (written through memcpy: the host mirror asks no alignment of `out`)
    for (size_t i = 0; i < n; ++i) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[i] : spp);
        double y[3];
        for (size_t c = 0; c < 3; ++c) {
            const double m = values[3 * i + c] * inv;
            const double x = m * scale;
            y[c] = rtm::rt_tonemap(p.op, x, w2);
        }
        if (format == RT_FILM_RGBE) {
            const uint32_t word = rtm::rt_rgbe_pack(y[0], y[1], y[2]);
            memcpy(bytes + 4 * i, &word, 4);
        } else if (format == RT_FILM_F32) {
            const uint32_t bits[3] = {rtm::rt_f32_of(y[0]), rtm::rt_f32_of(y[1]), rtm::rt_f32_of(y[2])};
            memcpy(bytes + 12 * i, bits, 12);
        } else {
            const uint16_t q[3] = {rtm::rt_quantise16(rtm::rt_gamma_encode(y[0])), rtm::rt_quantise16(rtm::rt_gamma_encode(y[1])),
                                   rtm::rt_quantise16(rtm::rt_gamma_encode(y[2]))};
            memcpy(bytes + 6 * i, q, 6);
        }
    }
    return 0;
}

// ---- bloom: the host mirror of rt_bloom_device (include/rt_amd.h "bloom") ----

int rth_bloom(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map, const rt_bloom_params *params,
              double *out_mean) {
    const std::string who("rth_bloom");
    rt_bloom_params p;
    if (const char *bad = rtbl::bad_argument(false, width, height, values, out_mean, nullptr, spp, params, p)) return fail(who + ": " + bad);
    const size_t w = (size_t)width, h = (size_t)height, n = w * h;
    {
        const char *lo = (const char *)values, *out = (const char *)out_mean;
        if (out < lo + n * 24u && lo < out + n * 24u) return fail(who + ": out_mean must not overlap values");
    }
    std::vector<double> b(3 * n), hh(3 * n), a(3 * n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[i] : spp);
        rtm::rt_bloom_bright(values[3 * i] * inv, values[3 * i + 1] * inv, values[3 * i + 2] * inv, p.threshold, &b[3 * i]);
    }
    // one five-tap accumulation per value of `dst`, from `src` along pixels (step 1, length w) or along rows (step w, length h)
    auto pass = [&](const std::vector<double> &src, std::vector<double> &dst, size_t stride, bool along_rows) {
        for (size_t j = 0; j < h; ++j)
            for (size_t i = 0; i < w; ++i)
                for (size_t c = 0; c < 3; ++c) {
                    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                    uint32_t inside = 0;
                    for (int d = 0; d < 5; ++d) {
                        const int64_t off = (int64_t)stride * (d - 2), ii = (int64_t)i + (along_rows ? 0 : off), jj = (int64_t)j + (along_rows ? off : 0);
                        if (ii < 0 || ii >= (int64_t)w || jj < 0 || jj >= (int64_t)h) continue;
                        inside |= 1u << d;
                        v[d] = src[3 * ((size_t)jj * w + (size_t)ii) + c];
                    }
                    dst[3 * (j * w + i) + c] = rtm::rt_bloom_taps(v, inside);
                }
    };
    for (int32_t k = 0; k < p.levels; ++k) {
        pass(b, hh, (size_t)1 << k, false);
        pass(hh, b, (size_t)1 << k, true);
        for (size_t e = 0; e < 3 * n; ++e) a[e] = a[e] + b[e];
    }
    for (size_t i = 0; i < n; ++i) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[i] : spp);
        for (size_t c = 0; c < 3; ++c) out_mean[3 * i + c] = rtm::rt_bloom_output(values[3 * i + c] * inv, a[3 * i + c], p.levels, p.strength);
    }
    return 0;
}

// ---- guided upsampling: the host mirror of rt_upsample_device (include/rt_amd.h "guided upsampling") ----

int rth_upsample(int32_t width, int32_t height, const double *low, int32_t spp, const double *albedo_sum, int32_t albedo_spp, const double *edge_sum,
                 int32_t edge_spp, const rt_upsample_params *params, double *out_mean, uint8_t *out_rgba8) {
    const std::string who("rth_upsample");
    rt_upsample_params p;
    if (const char *bad = rtup::bad_argument(false, width, height, low, out_mean, nullptr, spp, albedo_sum, albedo_spp, edge_sum, edge_spp, params, p))
        return fail(who + ": " + bad);
    if (const char *bad = rtup::bad_overlap(false, width, height, p.factor, out_mean, low, albedo_sum, edge_sum)) return fail(who + ": " + bad);
    const int32_t F = p.factor, lw = rtm::rt_up_low_size(width, F), lh = rtm::rt_up_low_size(height, F);
    const size_t n_low = (size_t)lw * (size_t)lh;
    std::vector<double> rec_r(4 * n_low), rec_a(albedo_sum ? 4 * n_low : 0), rec_g(edge_sum ? 4 * n_low : 0);
    const double inv_spp = 1.0 / (double)spp, n_a = (double)albedo_spp, n_e = (double)edge_spp;
    for (int32_t J = 0; J < lh; ++J)
        for (int32_t I = 0; I < lw; ++I) {
            const size_t q = ((size_t)J * (size_t)lw + (size_t)I) * 4u;
            rtm::rt_upsample_prepare(I, J, width, height, F, low, inv_spp, albedo_sum, n_a, edge_sum, n_e, p.albedo_floor, &rec_r[q],
                                     albedo_sum ? &rec_a[q] : nullptr, edge_sum ? &rec_g[q] : nullptr);
        }
    const rtm::UpsampleRegions regions{rec_r.data(), rec_a.data(), rec_g.data(), lw};
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) {
            const size_t px = (size_t)y * (size_t)width + (size_t)x;
            double ap[3] = {0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0}, *out = out_mean + 3 * px;
            for (int k = 0; k < 3; ++k) {
                if (albedo_sum) ap[k] = albedo_sum[3 * px + k] / n_a;
                if (edge_sum) gp[k] = edge_sum[3 * px + k] / n_e;
            }
            if (albedo_sum && edge_sum) rtm::rt_upsample_pixel<true, true>(x, y, F, lw, lh, ap, gp, p.sigma_albedo, p.sigma_edge, p.albedo_floor, regions, regions, out);
            else if (albedo_sum) rtm::rt_upsample_pixel<true, false>(x, y, F, lw, lh, ap, gp, p.sigma_albedo, p.sigma_edge, p.albedo_floor, regions, regions, out);
            else if (edge_sum) rtm::rt_upsample_pixel<false, true>(x, y, F, lw, lh, ap, gp, p.sigma_albedo, p.sigma_edge, p.albedo_floor, regions, regions, out);
            else rtm::rt_upsample_pixel<false, false>(x, y, F, lw, lh, ap, gp, p.sigma_albedo, p.sigma_edge, p.albedo_floor, regions, regions, out);
            if (out_rgba8) {
                const uint32_t word = rtm::rt_upsample_rgba8(out);
                for (int k = 0; k < 4; ++k) out_rgba8[4 * px + (size_t)k] = (uint8_t)(word >> (8 * k));
            }
        }
    return 0;
}

// ---- robust frames: the host mirror of rt_robust_device (include/rt_amd.h "robust frames") ----

int rth_robust(int32_t width, int32_t height, int32_t blocks, const double *stack, int32_t spp, const rt_robust_params *params, double *out_mean,
               double *out_m2) {
    const std::string who("rth_robust");
    rt_robust_params p;
    if (const char *bad = rtrb::bad_argument(false, width, height, blocks, stack, out_mean, spp, params, p)) return fail(who + ": " + bad);
    if (const char *bad = rtrb::bad_overlap(false, width, height, blocks, stack, out_mean, out_m2)) return fail(who + ": " + bad);
    const size_t total = (size_t)width * (size_t)height * 3u;
    const rtrb::Rule rule = rtrb::rule_of(p, blocks, spp);
    // the form the device's built-in rule takes for this K (any larger one gives the same bits)
    double (*one)(const double *, size_t, const rtrb::Rule &, double *) = nullptr;
    switch (rtrb::kmax_for(blocks)) {
    case 4: one = rtrb::combine_strided<4>; break;
    case 8: one = rtrb::combine_strided<8>; break;
    case 16: one = rtrb::combine_strided<16>; break;
    default: one = rtrb::combine_strided<32>; break;
    }
    for (size_t e = 0; e < total; ++e) {
        double m2 = 0.0;
        out_mean[e] = one(stack + e, total, rule, out_m2 ? &m2 : nullptr);
        if (out_m2) out_m2[e] = m2;
    }
    return 0;
}

// ---- panoramas: the host mirror of rt_panorama_device (include/rt_amd.h "panoramas") ----

int rth_panorama(int32_t width, int32_t height, const double *tables, const double *faces, int32_t face_size, int32_t guard, int32_t spp,
                 double *out_mean) {
    if (const char *bad = rtpn::bad_argument(false, width, height, tables, faces, face_size, guard, spp, out_mean))
        return fail(std::string("rth_panorama: ") + bad);
    rtpn::resample(width, height, tables, faces, face_size, guard, spp, out_mean);
    return 0;
}

// ---- frame metrics: the host mirrors of rt_frame_error_device and rt_frame_noise_device (include/rt_amd.h "frame metrics") ----

extern "C++" {
namespace {
template <int A> struct MetricsEntry { double e[A]; uint32_t count; };

// the normative reduction over records: 256 entries per block (the last one padded with the neutral entry), each block by the tree
// `for stride = 128 .. 1: e[i] = e[i] (+) e[i + stride]`, the block results the next level's entries, until one is left
template <int A, class Combine>
MetricsEntry<A> reduce_metrics(std::vector<MetricsEntry<A>> entries, Combine combine) {
    for (;;) {
        const size_t blocks = (entries.size() + 255u) / 256u;
        std::vector<MetricsEntry<A>> next(blocks);
        for (size_t b = 0; b < blocks; ++b) {
            MetricsEntry<A> e[256];
            for (size_t i = 0; i < 256; ++i) e[i] = b * 256u + i < entries.size() ? entries[b * 256u + i] : MetricsEntry<A>{};
            for (size_t stride = 128; stride >= 1; stride >>= 1)
                for (size_t i = 0; i < stride; ++i) combine(e[i].e, &e[i].count, e[i + stride].e, e[i + stride].count);
            next[b] = e[0];
        }
        if (blocks == 1) return next[0];
        entries.swap(next);
    }
}
} // namespace
} // extern "C++"

int rth_frame_error(int32_t width, int32_t height, const double *values, int32_t spp, const int32_t *spp_map, const double *ref, int32_t ref_spp,
                    const rt_frame_error_params *params, double *out8) {
    rt_frame_error_params p;
    if (const char *bad = rtmt::bad_error_argument(false, width, height, values, spp, ref, ref_spp, params, out8, nullptr, p))
        return fail(std::string("rth_frame_error: ") + bad);
    const size_t n = (size_t)width * (size_t)height;
    const double inv_ref = 1.0 / (double)ref_spp;
    std::vector<MetricsEntry<rtm::RT_ERROR_ACCS>> terms(n);
    for (size_t i = 0; i < n; ++i) {
        const double inv = 1.0 / (double)(spp_map ? spp_map[i] : spp);
        const double m[3] = {values[3 * i] * inv, values[3 * i + 1] * inv, values[3 * i + 2] * inv};
        const double r[3] = {ref[3 * i] * inv_ref, ref[3 * i + 1] * inv_ref, ref[3 * i + 2] * inv_ref};
        rtm::rt_error_term(m, r, p.eps, terms[i].e, &terms[i].count);
    }
    const auto total = reduce_metrics<rtm::RT_ERROR_ACCS>(std::move(terms), rtm::rt_error_combine);
    rtm::rt_error_result(total.e, total.count, p.peak, out8);
    return 0;
}

int rth_frame_noise(int32_t width, int32_t height, int32_t form, const double *a, const double *b, int32_t n, const int32_t *spp_map,
                    const rt_frame_noise_params *params, double *out4) {
    rt_frame_noise_params p;
    if (const char *bad = rtmt::bad_noise_argument(false, width, height, form, a, b, n, spp_map, params, out4, nullptr, p))
        return fail(std::string("rth_frame_noise: ") + bad);
    const size_t pixels = (size_t)width * (size_t)height;
    std::vector<MetricsEntry<rtm::RT_NOISE_ACCS>> terms(pixels);
    for (size_t i = 0; i < pixels; ++i)
        rtm::rt_noise_term(form == RT_METRICS_MEANS, a + 3 * i, b + 3 * i, spp_map ? spp_map[i] : n, p.eps, terms[i].e, &terms[i].count);
    const auto total = reduce_metrics<rtm::RT_NOISE_ACCS>(std::move(terms), rtm::rt_noise_combine);
    rtm::rt_noise_result(total.e, total.count, out4);
    return 0;
}

int rth_read_pfm(const char *path, int32_t *out_width, int32_t *out_height, double *out_rgb, int64_t capacity) {
    if (!path || !out_width || !out_height) return fail("rth_read_pfm: null argument");
    try {
        std::vector<double> px;
        const std::string bad = read_pfm_rgb(path, *out_width, *out_height, out_rgb ? &px : nullptr);
        if (!bad.empty()) return fail("rth_read_pfm: " + bad);
        if (out_rgb) {
            if ((int64_t)px.size() > capacity) return fail("rth_read_pfm: buffer too small");
            memcpy(out_rgb, px.data(), px.size() * sizeof(double));
        }
        return 0;
    } catch (const std::exception &e) {
        return fail(std::string("rth_read_pfm: ") + e.what());
    }
}

int rth_write_png(const char *path, int32_t width, int32_t height, const uint8_t *rgb8) {
    if (!path || !rgb8) return fail("rth_write_png: null argument");
    return write_png_rgb8(path, width, height, rgb8) ? 0 : fail(std::string("rth_write_png: cannot write ") + path);
}

int rth_write_hdr(const char *path, int32_t width, int32_t height, const uint8_t *rgbe) {
    if (!path || !rgbe) return fail("rth_write_hdr: null argument");
    return write_hdr_rgbe(path, width, height, rgbe) ? 0 : fail(std::string("rth_write_hdr: cannot write ") + path);
}

int rth_write_pfm(const char *path, int32_t width, int32_t height, const float *rgb_f32) {
    if (!path || !rgb_f32) return fail("rth_write_pfm: null argument");
    return write_pfm_rgb(path, width, height, rgb_f32) ? 0 : fail(std::string("rth_write_pfm: cannot write ") + path);
}

int rth_write_png16(const char *path, int32_t width, int32_t height, const uint16_t *rgb16) {
    if (!path || !rgb16) return fail("rth_write_png16: null argument");
    return write_png_rgb16(path, width, height, rgb16) ? 0 : fail(std::string("rth_write_png16: cannot write ") + path);
}

int rth_synthetic_earth(int32_t width, int32_t height, uint8_t *out_rgb8) {
    if (!out_rgb8) return fail("rth_synthetic_earth: null argument");
    try {
        const ImageRGB8 img = synthetic_earth(width, height);
        memcpy(out_rgb8, img.pixels->data(), img.pixels->size());
        return 0;
    } catch (const std::exception &e) {
        return fail(e.what());
    }
}

int rth_load_image(const char *path, int32_t *out_width, int32_t *out_height, uint8_t *out_rgb8, int64_t capacity) {
    if (!path || !out_width || !out_height) return fail("rth_load_image: null argument");
    try {
        const ImageRGB8 img = load_image_rgb8(path);
        *out_width = img.width;
        *out_height = img.height;
        if (out_rgb8) {
            if ((int64_t)img.pixels->size() > capacity) return fail("rth_load_image: buffer too small");
            memcpy(out_rgb8, img.pixels->data(), img.pixels->size());
        }
        return 0;
    } catch (const std::exception &e) {
        return fail(e.what());
    }
}

} // extern "C"
