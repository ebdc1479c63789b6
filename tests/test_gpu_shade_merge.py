"""The shade round's shared work (rt_kernel.hip, `run == ST_SHADE`): one normalize per round on an operand selected per lane (the
ray's direction for Metal and Dielectric, the unit-sphere sample for Lambertian and Isotropic) in the spheres-only kernels, the
branches' own normalizes in every other family.  The merged value is the same function of the same operand, so every frame must stay
what the CPU oracle renders, bit for bit (u64 views of the f64 sums) — in every family, whichever form of the block it compiles.

One hand-made scene per family of kernels that compiles the shade block differently — spheres only, textures, quads + frames, every
feature (with ConstantMedia: Isotropic) — at 16x16 pixels, 4 samples, depth 8.  Each puts a Lambertian floor, a Metal with fuzz 0.3, a
Dielectric with a Lambertian body INSIDE it, and a DiffuseLight within two units of each other: the 64 lanes of a wave hold a mix of
them in nearly every shade round.  Each is seen through two cameras without defocus:
  "outside": from z = 9 towards the group; the glass is entered front_face and left from within.
  "inside":  from inside a second glass body, the view direction 47.8 degrees (sphere, the camera at 0.9 radii from the centre) or 42
             degrees (cube) off the outward normal.  With the 20 degree field of view the FIRST hit's angle of incidence then runs
             across the frame through the critical angle of 1.5 -> 1 (41.8 degrees: sin = 0.9 sin(47.8 +- 10) = 0.55 .. 0.76 against
             0.667 for the sphere, 32 .. 52 degrees for the cube's face): total reflection on one side of the frame, the Schlick draw
             on the other, front_face false, and no random number decides which
             (test_inside_views_straddle_the_critical_angle computes it from the camera).
rt_debug_last_kernel says which kernel ran.

The spheres-only scene is also rendered scaled by 2^-300 and by 2^+300 (every length of the scene and of the camera; a power of two
moves no mantissa): len2(d) is then near 2^-600 / 2^+600 of its usual size, so the square root and the divisions of normalize run
through the scaling paths of their expansions.  Exponent used: 300 both ways — the oracle alone renders both frames finite and
non-zero (asserted before the device is asked) — and 250 both ways beside them, where the large scene is still hit (see the tests).
t_min = 0.001 is NOT scaled, so the scaled frames are other frames than the unscaled one.

GPU time: 12 renders of 1024 samples; the oracle's frames are made once each."""
import math

import numpy as np
import pytest

import custom_scenes
from adaptive_helpers import assert_bits, bits

pytestmark = pytest.mark.gpu

W = H = 16
SPP, DEPTH = 4, 8
OUTSIDE = ((0.0, 1.0, 9.0), (0.0, 0.0, 0.0))
BODY = (1.8, 0.3, 2.5)  # the centre of the glass body the second camera sits in
_SPHERE_PHI, _CUBE_PHI = math.radians(47.8), math.radians(42.0)
INSIDE = {  # family -> (look_from, look_at): see the module's docstring
    "sphere": ((BODY[0] - 0.9, BODY[1], BODY[2]),
               (BODY[0] - 0.9 - 3.0 * math.cos(_SPHERE_PHI), BODY[1], BODY[2] - 3.0 * math.sin(_SPHERE_PHI))),
    "cube": (BODY, (BODY[0] - 3.0 * math.cos(_CUBE_PHI), BODY[1], BODY[2] - 3.0 * math.sin(_CUBE_PHI))),
}
FAMILIES = {  # name -> (rt_kernels.h feature mask, which glass body the inside camera is in)
    "spheres": (1, "sphere"),
    "textures": (19, "sphere"),
    "quads_frames": (6, "cube"),
    "all": (31, "sphere"),
}
_base, _scenes, _oracle = [], {}, {}


class _Aimed:
    def __init__(self, camera):
        self.camera = camera


def camera(rt, look, scale=1.0):
    """random-spheres' camera at 16x16 (20 degrees), aimed by `look`, without defocus; scale: every length times it"""
    if not _base:
        hs = rt.HostScene(0, width=W, aspect=1.0, spp=SPP, depth=DEPTH)
        assert (hs.width, hs.height) == (W, H)
        _base.append(hs)
    cam = rt.camera_look(_base[0], *look)
    cam.samples_per_pixel, cam.max_depth, cam.defocus_angle = SPP, DEPTH, 0.0
    cam.background = rt.Vec3(0.7, 0.8, 1.0)
    if scale != 1.0:
        for name in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v", "defocus_disk_u", "defocus_disk_v"):
            v = getattr(cam, name)
            setattr(cam, name, rt.Vec3(v.x * scale, v.y * scale, v.z * scale))
    return cam


def _cube(s, lo, hi, m):
    """a list of the six quads of Quad::cube, all of material m"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    return s.list([s.quad((x0, y0, z1), (dx, 0, 0), (0, dy, 0), m), s.quad((x1, y0, z1), (0, 0, -dz), (0, dy, 0), m),
                   s.quad((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), m), s.quad((x0, y0, z0), (0, 0, dz), (0, dy, 0), m),
                   s.quad((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), m), s.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), m)])


def scene(rt, family, scale=1.0):
    key = (family, scale)
    if key in _scenes:
        return _scenes[key]
    k = scale
    s = custom_scenes.CustomScene(_Aimed(camera(rt, OUTSIDE, scale)), spp=SPP, depth=DEPTH, background=(0.7, 0.8, 1.0))
    P = lambda x, y, z: (x * k, y * k, z * k)
    metal, glass, lamp = s.metal(0.8, 0.7, 0.5, 0.3), s.dielectric(1.5), s.light(4.0, 4.0, 4.0)
    body, small = s.lambertian(0.8, 0.3, 0.3), s.lambertian(0.3, 0.4, 0.8)
    if family in ("textures", "all"):
        img = s.image(s.add_image(custom_scenes.random_image(3, 13, 5)))
        floor = s.lambertian_tex(s.checker(0.6, s.solid(0.9, 0.9, 0.3), img))
        small = s.lambertian_tex(s.noise(4.0, s.add_perlin(custom_scenes.perlin_table_a())))
        lamp = s.light_tex(s.checker(0.5, s.solid(4.0, 4.0, 4.0), s.solid(2.0, 3.0, 4.0)))
    else:
        floor = s.lambertian(0.5, 0.6, 0.4)
    if family == "quads_frames":  # no sphere anywhere: every body is a cube of quads inside Translate(RotateY(...))
        items = [
            s.quad((-5.0, -1.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), floor),
            s.translate(s.rotate_y(_cube(s, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), metal), 25.0), (-0.9, -0.5, 0.0)),
            s.translate(s.rotate_y(_cube(s, (-0.6, -0.6, -0.6), (0.6, 0.6, 0.6), glass), -20.0), (0.9, -0.4, 0.0)),
            s.translate(s.rotate_y(_cube(s, (-0.3, -0.3, -0.3), (0.3, 0.3, 0.3), body), 40.0), (1.05, -0.4, 0.1)),  # inside the glass
            s.quad((-0.6, 1.6, -1.0), (1.2, 0.0, 0.0), (0.0, 0.3, 1.0), lamp),
            s.translate(_cube(s, (-0.25, -0.25, -0.25), (0.25, 0.25, 0.25), small), (0.0, -0.75, 0.9)),
            s.translate(_cube(s, (-1.0, -1.0, -2.0), (1.0, 1.0, 2.0), glass), BODY),  # the inside camera's: axis-aligned
            s.translate(s.rotate_y(s.quad((-0.3, -0.3, 0.0), (0.6, 0.0, 0.0), (0.0, 0.6, 0.0), body), 30.0), (BODY[0] + 0.3, BODY[1], BODY[2] + 1.0)),
        ]
    else:
        items = [
            s.sphere(P(0.0, -1001.0, 0.0), 1000.0 * k, floor),
            s.sphere(P(-0.9, -0.4, 0.0), 0.6 * k, metal),
            s.sphere(P(0.9, -0.3, 0.0), 0.7 * k, glass),
            s.sphere(P(1.1, -0.3, 0.0), 0.35 * k, body),  # inside the glass, off its centre: its scatter meets the glass at every angle
            s.sphere(P(0.0, 1.2, -0.5), 0.5 * k, lamp),
            s.sphere(P(0.0, -0.7, 0.9), 0.3 * k, small),
            s.sphere(P(*BODY), 1.0 * k, glass),           # the inside camera's
            s.sphere(P(BODY[0] + 0.4, BODY[1], BODY[2] + 0.3), 0.3 * k, body),
        ]
        if family in ("textures", "all"):
            items.append(s.quad((-0.6, 1.9, -1.0), (1.2, 0.0, 0.0), (0.0, 0.0, 1.0), lamp))
        if family == "all":
            items.append(s.translate(s.rotate_y(_cube(s, (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4), metal), 30.0), (-0.2, 0.3, -1.2)))
            items.append(s.medium(s.sphere((-0.9, -0.4, 0.0), 1.1, glass), 1.2, 0.6, 0.7, 0.9))      # a haze around the Metal
            items.append(s.medium(s.translate(_cube(s, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), body), (0.3, -0.5, 1.6)), 2.5,
                                  texture=s.checker(0.3, s.solid(0.9, 0.5, 0.2), s.solid(0.2, 0.5, 0.9))))
    _scenes[key] = s.finish(s.list(items))
    return _scenes[key]


def oracle_frame(rt, oracle, hs, key, cam, seed):
    if key not in _oracle:
        f = oracle.render(hs, rt.render_params(seed=seed), camera=cam)
        f.setflags(write=False)
        _oracle[key] = f
    return _oracle[key]


def check(rt, oracle, family, view, scale=1.0, seed=11, min_values=9):
    feat, body_kind = FAMILIES[family]
    hs = scene(rt, family, scale)
    # (the camera is built at unit scale and its lengths multiplied: exact, and no 2^300-sized vector is squared on the way)
    cam = camera(rt, OUTSIDE if view == "outside" else INSIDE[body_kind], scale)
    want = oracle_frame(rt, oracle, hs, (family, view, scale, seed), cam, seed)
    # the oracle alone first: a frame of finite values, not all of them zero, and of at least min_values different ones
    assert np.isfinite(want).all() and want.max() > 0.0, (family, view, scale)
    assert len(np.unique(bits(want))) >= min_values, (family, view, scale, "the frame checks less than it says")
    got = rt.DeviceScene(hs, walk=rt.RT_WALK_OWN_TREES, wide=1).render(rt.render_params(seed=seed), camera=cam)
    # the library's own trees, four-child records, the scene and its small tables in the LDS: for the spheres-only scene that is the
    # kernel class of the flagship workload
    assert rt.debug_last_kernel() == dict(features=feat, lds_level=3, ordered=1, wide=1, aux=1, jobs=rt.RT_JOBS_DENSE, ids_ok=1, threads=1024), family
    assert_bits(got, want, f"{family} scene from {view}, scale {scale!r}")


@pytest.mark.parametrize("view", ["outside", "inside"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_material_in_one_wave_matches_the_oracle(rt, oracle, gpu, family, view):
    check(rt, oracle, family, view)


@pytest.mark.parametrize("body_kind", ["sphere", "cube"])
def test_inside_views_straddle_the_critical_angle(rt, body_kind):
    """What the module's docstring argues from geometry, computed: the rays through the pixel centres of the "inside" camera leave its
    glass body (a unit sphere about BODY / the cube BODY + [-1, 1] x [-1, 1] x [-2, 2], through its -x face) with 1.5 sin(incidence)
    well above 1 in at least 16 pixels (total reflection, whatever is drawn) and well below 1 in at least 16 (the Schlick draw)."""
    cam = camera(rt, INSIDE[body_kind])
    vec = lambda v: np.array([v.x, v.y, v.z])
    o, p00, du, dv = vec(cam.center), vec(cam.pixel00_loc), vec(cam.pixel_delta_u), vec(cam.pixel_delta_v)
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    d = p00 + i[..., None] * du + j[..., None] * dv - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    c = o - np.array(BODY)
    if body_kind == "sphere":
        assert np.linalg.norm(c) < 1.0  # the camera is inside: the first hit is the exit, at the line's distance from the centre
        sin_i = np.linalg.norm(np.cross(np.broadcast_to(c, d.shape), d), axis=-1) / 1.0
    else:
        t = (-1.0 - c[0]) / d[..., 0]  # the -x face
        at = c + t[..., None] * d
        assert (d[..., 0] < 0).all() and (np.abs(at[..., 1]) < 1.0).all() and (np.abs(at[..., 2]) < 2.0).all(), "some ray leaves through another face"
        sin_i = np.sqrt(1.0 - d[..., 0] ** 2)
    assert (1.5 * sin_i > 1.05).sum() >= 16 and (1.5 * sin_i < 0.95).sum() >= 16, (body_kind, np.sort(1.5 * sin_i.ravel())[[0, -1]])


@pytest.mark.parametrize("exponent", [-300, 300])
def test_spheres_scene_scaled_by_a_large_power_of_two(rt, oracle, gpu, exponent):
    """Exponent 300 in both directions: the oracle's frames at 2^-300 and 2^+300 are finite and non-zero (check asserts it), so the
    exponent was not reduced.  What they hold, on the CPU: at 2^-300 every camera ray hits and is shaded once — Metal and Dielectric
    normalize a direction of squared length near 2^-594 — and the scattered ray's t_min leaps over the scene (13 different values);
    at 2^+300 Sphere::hit's a * c overflows for every camera ray (2^606 x 2^606 and more), the discriminant is inf - inf, nothing is
    hit and the frame is the background's three values: it stays as a case of the very large squared length that reaches no shade
    round.  The case below is the one that does."""
    check(rt, oracle, "spheres", "outside", scale=math.ldexp(1.0, exponent), min_values=3)


@pytest.mark.parametrize("exponent", [-250, 250])
def test_spheres_scene_at_the_largest_scale_that_is_still_hit(rt, oracle, gpu, exponent):
    """2^+250 is the largest power of two (to a few units) at which a * c of a camera ray stays below 2^1024 for the ground sphere
    (81 x 2^500 x 10^6 x 2^500): camera rays hit, are shaded, scatter and hit again (300 different values on the CPU).  2^-250 beside
    it for symmetry."""
    check(rt, oracle, "spheres", "outside", scale=math.ldexp(1.0, exponent))
