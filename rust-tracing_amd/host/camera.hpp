// CameraSettings and Camera::new, host side.  get_ray runs on the GPU (csrc/rt_kernel.hip).
//   reference: src/camera.rs:8-110
#pragma once
#include "vec3.hpp"

namespace rt {

struct CameraSettings { // defaults: src/camera.rs:21-37
    FP aspect_ratio = 16.0 / 9.0;
    size_t image_width = 400;
    int32_t samples_per_pixel = 100;
    int32_t max_depth = 50;
    FP vfov = 90.0;
    Point3 look_from = Point3::ZERO();
    Point3 look_at = Point3(0.0, 0.0, -1.0);
    Vec3 vup = Vec3::UP();
    FP defocus_angle = 0.0;
    FP focus_dist = 10.0;
    Color background = Color::ZERO();
};

// look_from turned about the axis through look_at along vup by 360 k / n degrees (rtrace --orbit, rth_scene_orbit_look_from): theta = 2 pi k / n; a = vup / |vup|; p = look_from - look_at;
// p' = p cos(theta) + (a x p) sin(theta) + a ((a . p) (1 - cos(theta))); result = look_at + p'.  k = 0 is look_from itself.
inline Point3 orbit_look_from(const Point3 &look_from, const Point3 &look_at, const Vec3 &vup, int k, int n) {
    if (k == 0) return look_from;
    const FP theta = 2.0 * 3.14159265358979323846264338327950288 * (FP)k / (FP)n;
    const FP c = std::cos(theta), s = std::sin(theta);
    const FP len = std::sqrt(vup.x * vup.x + vup.y * vup.y + vup.z * vup.z);
    const FP ax = vup.x / len, ay = vup.y / len, az = vup.z / len;
    const FP px = look_from.x - look_at.x, py = look_from.y - look_at.y, pz = look_from.z - look_at.z;
    const FP cx = ay * pz - az * py, cy = az * px - ax * pz, cz = ax * py - ay * px;
    const FP t = (ax * px + ay * py + az * pz) * (1.0 - c);
    return Point3(look_at.x + (px * c + cx * s + ax * t), look_at.y + (py * c + cy * s + ay * t), look_at.z + (pz * c + cz * s + az * t));
}

class Camera {
  public:
    size_t image_width, image_height;
    int32_t samples_per_pixel, max_depth;
    Color background;
    CameraSettings settings; // what this camera was made from: another view of the scene is Camera(settings with other look points)

    explicit Camera(const CameraSettings &s) {
        settings = s;
        image_width = s.image_width;
        samples_per_pixel = s.samples_per_pixel;
        max_depth = s.max_depth;
        background = s.background;

        image_height = (size_t)((FP)image_width / s.aspect_ratio); // `as usize` truncation (src/camera.rs:69)

        const FP theta = degrees_to_radians(s.vfov);
        const FP h = std::tan(theta / 2.0);

        const FP viewport_height = 2.0 * h * s.focus_dist;
        const FP viewport_width = viewport_height * ((FP)image_width / (FP)image_height);

        const Vec3 w = (s.look_from - s.look_at).normalize();
        const Vec3 u = s.vup.cross(w).normalize();
        const Vec3 v = w.cross(u);

        const Vec3 viewport_u = viewport_width * u;
        const Vec3 viewport_v = -viewport_height * v;

        center = s.look_from;
        pixel_delta_u = viewport_u / (FP)image_width;
        pixel_delta_v = viewport_v / (FP)image_height;

        const Vec3 viewport_upper_left = center - s.focus_dist * w - viewport_u * 0.5 - viewport_v * 0.5;
        pixel00_loc = viewport_upper_left + 0.5 * (pixel_delta_u + pixel_delta_v);

        defocus_angle = s.defocus_angle;
        const FP defocus_radius = s.focus_dist * std::tan(degrees_to_radians(s.defocus_angle / 2.0));
        defocus_disk_u = u * defocus_radius;
        defocus_disk_v = v * defocus_radius;
    }

    rt_camera pod() const {
        rt_camera c{};
        c.image_width = (int32_t)image_width;
        c.image_height = (int32_t)image_height;
        c.samples_per_pixel = samples_per_pixel;
        c.max_depth = max_depth;
        c.background = background.pod();
        c.center = center.pod();
        c.pixel00_loc = pixel00_loc.pod();
        c.pixel_delta_u = pixel_delta_u.pod();
        c.pixel_delta_v = pixel_delta_v.pod();
        c.defocus_angle = defocus_angle;
        c.defocus_disk_u = defocus_disk_u.pod();
        c.defocus_disk_v = defocus_disk_v.pod();
        return c;
    }

  private:
    Point3 center, pixel00_loc;
    Vec3 pixel_delta_u, pixel_delta_v;
    FP defocus_angle;
    Vec3 defocus_disk_u, defocus_disk_v;
};

} // namespace rt
