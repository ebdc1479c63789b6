"""The inline start test (rt_kernel.hip, where a query starts): when the start shortcut's leaf is a single sphere, that sphere's
Sphere::hit runs for the lanes that start a query, right there, instead of in a round of the sphere stage (KParams::start_inline;
RT_START_INLINE, rt_debug_set_start_inline; default on).

Every frame here is held to the CPU oracle bit for bit (u64 views of the f64 sums), with the knob on and off.  Frames are 44x28 (6x4
tiles, ragged to the right and at the bottom) at 4-6 samples (40 for the render of several launches), depth 10.

Whether a render really took the inline test is read from a counted render: a round of the sphere stage adds its lanes to the stage
profile, one per test, and every query makes exactly one start test.  So the lanes of the sphere stage are sphere_tests with the
test in the stage and sphere_tests - rays with the test inline; anything else fails.

The hand-made scene: a ground sphere of radius 1000 (top at y = 0) under 70 small spheres, one of them tangent to the ground, and
around a lamp; seen from outside, from INSIDE the ground (the first root lies behind the origin, the second decides), from a point exactly ON its surface
(c = 0: a root at 0, below t_min) and from half a millimetre above it (roots on either side of t_min = 0.001); rays over the horizon
miss it with a negative discriminant.  Variants: the ground MOVES (center_vec, a time per path); a second sphere COINCIDES with the
ground (leaf_max 1 keeps the start leaf at one sphere: every later hit of the twin ties with the start sphere already the closest).

GPU time, measured on an MI355X: 12.6 s for the file run alone (19 cases), 11.5 s of it the process's first use of torch and the
device (paid once in the whole suite anyway); no other case above 0.2 s."""
import os
import random

import numpy as np
import pytest

import custom_scenes
import scene_cases
from adaptive_helpers import SENTINEL, assert_bits, bits, launches_for, tile_order

pytestmark = pytest.mark.gpu

W, H, DEPTH = 44, 28, 10
LOOKS = {  # name -> (look_from, look_at, defocus kept?)
    "outside": ((6.0, 2.0, 9.0), (0.0, 0.3, 0.0), True),
    "inside": ((-4.0, -2.0, 9.0), (0.0, -1.0, 0.0), True),
    "on_surface": ((0.0, 0.0, 0.0), (3.0, 0.0, -5.0), False),
    "grazing": ((0.0, 0.0005, 4.0), (0.5, 0.0, -5.0), False),
}
_base, _scenes, _oracle = [], {}, {}


class _Aimed:
    def __init__(self, camera):
        self.camera = camera


def base_scene(rt):
    """random-spheres at 44x28: scene 0 itself, and the camera every hand-made scene here is seen through"""
    if not _base:
        hs = rt.HostScene(0, width=W, aspect=W / H, spp=6, depth=DEPTH)
        assert (hs.width, hs.height) == (W, H)
        _base.append(hs)
    return _base[0]


def look(rt, name, spp):
    look_from, look_at, defocus = LOOKS[name]
    cam = rt.camera_look(base_scene(rt), look_from, look_at)
    cam.samples_per_pixel, cam.max_depth = spp, DEPTH
    if not defocus:
        cam.defocus_angle = 0.0  # every ray starts at look_from exactly
    return cam


def ground_scene(rt, variant, n_small=70, spp=4):
    """variant: "still" | "moving" | "twin" (see the module's docstring) | "small" (20 small spheres: fewer than 64 primitives)"""
    key = (variant, n_small, spp)
    if key in _scenes:
        return _scenes[key]
    rnd = random.Random(17)
    s = custom_scenes.CustomScene(_Aimed(look(rt, "outside", spp)), spp=spp, depth=DEPTH, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(6)]
    mats += [s.metal(0.8, 0.7, 0.6, 0.0), s.metal(0.6, 0.8, 0.7, 0.2), s.dielectric(1.5), s.light(3, 3, 3)]
    items = [s.sphere((0.0, -1000.0, 0.0), 1000.0, mats[0])]
    if variant == "moving":
        s.spheres[0].center_vec, s.spheres[0].is_moving = rt.Vec3(0.0, 0.4, 0.0), 1
    items.append(s.sphere((0.5, 0.5, 0.5), 0.5, mats[6]))  # tangent to the still ground at (0.5, 0, 0.5)
    items.append(s.sphere((0.5, -6.0, 3.0), 3.0, s.light(6, 6, 6)))  # a lamp INSIDE the ground: what a camera in there sees by
    for _ in range(n_small - 1):
        r = rnd.uniform(0.1, 0.4)
        items.append(s.sphere((rnd.uniform(-5, 5), r + rnd.choice([0.0, 0.0, rnd.uniform(0.0, 1.5)]), rnd.uniform(-5, 5)), r, rnd.choice(mats)))
    if variant == "twin":
        items.append(s.sphere((0.0, -1000.0, 0.0), 1000.0, mats[7]))
    _scenes[key] = s.finish(s.list(items))
    return _scenes[key]


def oracle_frame(rt, oracle, hs, tag, camera=None, **params):
    key = (tag, bytes(camera) if camera is not None else None, tuple(sorted(params.items())))
    if key not in _oracle:
        f = oracle.render(hs, rt.render_params(**params), camera=camera)
        f.setflags(write=False)
        _oracle[key] = f
    return _oracle[key]


class inline:
    """with inline(rt, v): renders inside run with start_inline = v; the process default comes back afterwards"""
    def __init__(self, rt, value):
        self.rt, self.value = rt, value

    def __enter__(self):
        assert self.rt.amd_lib().rt_debug_set_start_inline(self.value) == 0

    def __exit__(self, *exc):
        self.rt.amd_lib().rt_debug_set_start_inline(int(os.environ.get("RT_START_INLINE", "1")))


def counted(rt, ds, cam, params):
    """(frame, counters, lanes the sphere stage's rounds served) of a counted render"""
    import ctypes as C
    import torch
    d = torch.zeros(cam.image_width * cam.image_height * 3, dtype=torch.float64, device="cuda")
    c = ds.render_device_counted(params, d.data_ptr(), torch.cuda.current_stream().cuda_stream, camera=cam)
    torch.cuda.synchronize()
    buf = (C.c_uint64 * 36)()
    assert rt.amd_lib().rt_debug_stage_profile(buf) == 0
    return d.cpu().numpy(), c, int(buf[3 * 1 + 1])


def assert_where_the_start_test_ran(rt, ds, cam, params, want, what):
    """the start test ran inline with the knob on and in the sphere stage with it off; both frames equal `want`"""
    with inline(rt, 1):
        f1, c1, lanes1 = counted(rt, ds, cam, params)
    with inline(rt, 0):
        f0, c0, lanes0 = counted(rt, ds, cam, params)
    assert_bits(f1, want, f"{what}: counted render, start test inline")
    assert_bits(f0, want, f"{what}: counted render, start test in the sphere stage")
    assert c1 == c0, what
    assert c1["rays"] > 0 and c1["sphere_tests"] >= c1["rays"], (what, c1)
    assert lanes0 == c0["sphere_tests"], (what, "knob off: every sphere test is a lane of a sphere round", lanes0, c0)
    assert lanes1 == c1["sphere_tests"] - c1["rays"], (what, "knob on: one test per query is made where the query starts", lanes1, c1)


def test_random_spheres_with_the_test_inline_in_the_stage_and_without_the_shortcut(rt, oracle, gpu):
    hs = base_scene(rt)
    params = rt.render_params(seed=5)
    want = oracle_frame(rt, oracle, hs, "scene0", seed=5)
    ds = rt.DeviceScene(hs)
    with inline(rt, 1):
        on = ds.render(params)
    assert rt.debug_last_kernel() == dict(features=rt.RT_FEAT_SPHERES_SOLID, lds_level=3, ordered=1, wide=1, aux=1, jobs=0, ids_ok=1, threads=1024)
    start = rt.debug_last_start()
    assert start["stage"] == 1 and start["end"] == start["first"] + 1 and start["start_inline"] == 1 and start["ran_inline"] == 1, start
    with inline(rt, 0):
        off = ds.render(params)
    assert rt.debug_last_start() == dict(start, start_inline=0, ran_inline=0)
    plain = rt.DeviceScene(hs, start_shortcut=0).render(params)
    assert rt.debug_last_start()["stage"] == 0 and rt.debug_last_start()["ran_inline"] == 0
    assert_bits(on, want, "random-spheres, start test inline")
    assert_bits(off, want, "random-spheres, start test in the sphere stage")
    assert_bits(plain, want, "random-spheres, no start shortcut")


def test_counted_renders_of_random_spheres_count_the_same_events(rt, oracle, gpu):
    hs = base_scene(rt)
    ds = rt.DeviceScene(hs)
    params = rt.render_params(seed=5)
    want = oracle_frame(rt, oracle, hs, "scene0", seed=5)
    assert_where_the_start_test_ran(rt, ds, hs.camera, params, want, "random-spheres")
    with inline(rt, 1):
        _, c1, _ = counted(rt, ds, hs.camera, params)
    with inline(rt, 0):
        _, c0, _ = counted(rt, ds, hs.camera, params)
    for name in ("samples", "rays", "node_visits", "sphere_tests", "rng_draws"):
        assert c1[name] == c0[name] and c1[name] > 0, (name, c1, c0)
    assert c1["samples"] == W * H * 6


@pytest.mark.parametrize("variant", ["still", "moving"])
@pytest.mark.parametrize("view", list(LOOKS))
def test_ground_sphere_scene_from_outside_inside_and_on_the_surface(rt, oracle, gpu, variant, view):
    hs = ground_scene(rt, variant)
    cam = look(rt, view, 4)
    cam.background = hs.camera.background
    params = rt.render_params(seed=7)
    want = oracle_frame(rt, oracle, hs, variant, camera=cam, seed=7)
    ds = rt.DeviceScene(hs)
    with inline(rt, 1):
        on = ds.render(params, camera=cam)
    assert rt.debug_last_kernel() == dict(features=rt.RT_FEAT_SPHERES_SOLID, lds_level=3, ordered=1, wide=1, aux=1, jobs=0, ids_ok=1, threads=1024)
    with inline(rt, 0):
        off = ds.render(params, camera=cam)
    assert_bits(on, want, f"{variant} ground from {view}, start test inline")
    assert_bits(off, want, f"{variant} ground from {view}, start test in the sphere stage")
    # (inside the still ground every path ends on the lamp or dies: a pixel's sum is one of a dozen values, not of one)
    assert len(np.unique(bits(want))) > 8, "the frame is (nearly) one colour: the view checks less than it says"
    if view == "inside":
        assert_where_the_start_test_ran(rt, ds, cam, params, want, f"{variant} ground from inside")


def test_a_twin_of_the_ground_ties_with_the_start_sphere(rt, oracle, gpu):
    hs = ground_scene(rt, "twin")
    params = rt.render_params(seed=9)
    ds = rt.DeviceScene(hs, leaf_max=1)
    for view in ("outside", "inside"):
        cam = look(rt, view, 4)
        cam.background = hs.camera.background
        want = oracle_frame(rt, oracle, hs, "twin", camera=cam, seed=9)
        assert_where_the_start_test_ran(rt, ds, cam, params, want, f"twin ground from {view}")
        assert rt.debug_last_kernel()["wide"] == 1
        # the twin is second in the reference's scan and a sphere: the first one keeps every tie.  Without the twin the frame is another
        single = oracle_frame(rt, oracle, ground_scene(rt, "still"), "still", camera=cam, seed=9)
        assert_bits(want, single, "oracle: the later of two coincident spheres never wins")


def test_fewer_than_64_primitives_take_the_inline_test_in_the_two_child_kernel(rt, oracle, gpu):
    hs = ground_scene(rt, "small", n_small=20)
    params = rt.render_params(seed=11)
    ds = rt.DeviceScene(hs)
    for view in ("outside", "inside"):
        cam = look(rt, view, 4)
        cam.background = hs.camera.background
        want = oracle_frame(rt, oracle, hs, "small", camera=cam, seed=11)
        assert_where_the_start_test_ran(rt, ds, cam, params, want, f"21 spheres from {view}")
        assert rt.debug_last_kernel() == dict(features=rt.RT_FEAT_SPHERES_SOLID, lds_level=3, ordered=1, wide=0, aux=1, jobs=0, ids_ok=1, threads=1024)


@pytest.mark.parametrize("value", [1, 0])
def test_list_mode_on_the_ground_scene(rt, oracle, gpu, value):
    import torch
    hs = ground_scene(rt, "moving")
    cam = look(rt, "inside", 4)
    cam.background = hs.camera.background
    want = oracle_frame(rt, oracle, hs, "moving", camera=cam, seed=7).reshape(W * H, 3)
    g = np.random.default_rng(3)
    pixels = tile_order(W, H)
    pixels = pixels[pixels != 0xFFFFFFFF]
    chosen = g.permutation(pixels)[:(W * H * 3) // 5].astype(np.uint32)  # 739 entries: no multiple of 64
    assert chosen.size % 64 != 0
    lst = torch.from_numpy(chosen.view(np.int32)).cuda()
    s = torch.full((W * H * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    ds = rt.DeviceScene(hs)
    with inline(rt, value):
        ds.render_pixels_device(rt.render_params(seed=7, sample_end=4), lst.data_ptr(), chosen.size, s.data_ptr(), 0,
                                torch.cuda.current_stream().cuda_stream, camera=cam)
        torch.cuda.synchronize()
    assert rt.debug_last_kernel()["jobs"] == rt.RT_JOBS_LIST and rt.debug_last_kernel()["features"] == rt.RT_FEAT_SPHERES_SOLID
    got = s.cpu().numpy().reshape(W * H, 3)
    mask = np.zeros(W * H, dtype=bool)
    mask[chosen] = True
    assert_bits(got[mask], want[mask], f"list mode, start_inline {value}")
    assert (bits(got[~mask]) == SENTINEL).all()


@pytest.mark.parametrize("value", [1, 0])
def test_views_mode_with_one_camera_inside_the_ground(rt, oracle, gpu, value):
    hs = ground_scene(rt, "still")
    views = (rt.View * 3)()
    for k, name in enumerate(("outside", "inside", "grazing")):
        cam = look(rt, name, 4)
        cam.background = hs.camera.background
        views[k].camera, views[k].seed = cam, 20 + k
    ds = rt.DeviceScene(hs)
    with inline(rt, value):
        got = ds.render_views(rt.render_params(sample_end=4), views)
    assert rt.debug_last_kernel()["jobs"] == rt.RT_JOBS_VIEWS and rt.debug_last_kernel()["features"] == rt.RT_FEAT_SPHERES_SOLID
    for k in range(3):
        want = oracle_frame(rt, oracle, hs, "still", camera=rt.Camera.from_buffer_copy(bytes(views[k].camera)), seed=20 + k)
        assert_bits(got[k].reshape(-1), want, f"views mode, start_inline {value}: view {k}")


def test_a_render_of_several_launches_and_a_continuation(rt, oracle, gpu):
    """a 1 MiB sample buffer holds 28 sample rows of the 24 tiles (14 per scratch set when launches overlap): 40 samples take several
    launches; then [0, 12) followed by [12, 40) with accumulate"""
    n = 40
    hs = ground_scene(rt, "moving")
    cam = look(rt, "inside", n)
    cam.background = hs.camera.background
    want = oracle_frame(rt, oracle, hs, "moving", camera=cam, seed=13, sample_end=n)
    budget = 1 << 20
    want_launches = launches_for(24 * 64, n, budget, os.environ.get("RT_OVERLAP", "1") != "0")[0]
    assert want_launches >= 2
    ds = rt.DeviceScene(hs, sample_buffer_bytes=budget)
    for value in (1, 0):
        with inline(rt, value):
            got = ds.render(rt.render_params(seed=13, sample_end=n), camera=cam)
            assert rt.debug_last_launch()["launches"] == want_launches
            assert_bits(got, want, f"{want_launches} launches, start_inline {value}")
            import torch
            d = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            ds.render_device(rt.render_params(seed=13, sample_begin=0, sample_end=12), d.data_ptr(), stream, camera=cam)
            ds.render_device(rt.render_params(seed=13, sample_begin=12, sample_end=n, accumulate=True), d.data_ptr(), stream, camera=cam)
            torch.cuda.synchronize()
            assert_bits(d.cpu().numpy(), want, f"[0, 12) + [12, {n}) with accumulate, start_inline {value}")


@pytest.mark.parametrize("case,kernel", [
    ("c3_cornell_box_64x64_16spp_d50", dict(features=6, lds_level=3, ordered=1, wide=0, aux=1, jobs=0, ids_ok=1, threads=1024)),
    ("cornell_smoke_64x64_16spp", dict(features=14, lds_level=3, ordered=1, wide=0, aux=1, jobs=0, ids_ok=1, threads=1024)),
])
def test_scenes_that_cannot_take_the_inline_test_are_untouched(rt, oracle, gpu, case, kernel):
    """Cornell starts with a leaf of quads, cornell_smoke has media: the knob changes nothing, not the kernel and not a bit"""
    hs = scene_cases.build(rt, case, width=32, spp=4, depth=DEPTH)
    assert (hs.width, hs.height) == (32, 32)
    want = oracle.render(hs, rt.render_params(seed=3))
    ds = rt.DeviceScene(hs)
    frames = []
    for value in (1, 0):
        with inline(rt, value):
            frames.append(ds.render(rt.render_params(seed=3)))
        assert rt.debug_last_kernel() == kernel, (case, value)
        assert rt.debug_last_start()["start_inline"] == 0 and rt.debug_last_start()["ran_inline"] == 0, (case, value, rt.debug_last_start())
    assert_bits(frames[0], frames[1], f"{case}: start_inline 1 against 0")
    assert_bits(frames[0], want, case)
