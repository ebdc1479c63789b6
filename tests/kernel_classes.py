"""Shared by tests/test_gpu_job_modes.py, tests/test_gpu_schedule.py and others (not a test module): one small scene per class of render kernel (rt_kernel.hip path_kernel's
LDS level x feature set x walk x record width x AUX, as rt_kernels.h path_kernel_for picks it), what rt_debug_last_kernel must report
for it, three views of every scene, and the pixel list of the list-mode stress shape.

The hand-made scenes (custom_scenes.py) lie around the origin; they are seen through the camera of ragged_cornell_37x37_4spp (37x37:
neither dimension a multiple of the 8x8 tile, 25 tiles) turned towards them with camera_look — where Cornell's own camera stands, none
of them is in the frame."""
import numpy as np

import custom_scenes
import scene_cases
from adaptive_helpers import PAD

CAMERA_CASE = "ragged_cornell_37x37_4spp"
LOOK_AT = (0.0, 0.0, 0.0)
LOOK_FROM = [(0.0, 0.0, 9.0), (4.5, 1.5, 7.5), (-5.0, 2.5, 6.5)]  # the scene's own camera, then two more views
MAX_DEPTH = 8

FEAT = dict(spheres_solid=1, quads_frames=6, quads_frames_media=14, spheres_quads_textures=19, all=31)  # rt_kernels.h FEAT_*
JOBS_LIST, JOBS_VIEWS = 1, 2

_camera_scene = []
_scenes = {}


class _Aimed:
    """what CustomScene takes its camera from"""
    def __init__(self, camera):
        self.camera = camera


def aimed_camera(rt, look_from):
    if not _camera_scene:
        _camera_scene.append(scene_cases.build(rt, CAMERA_CASE))
    cam = rt.camera_look(_camera_scene[0], look_from, LOOK_AT)
    assert (cam.image_width, cam.image_height) == (37, 37)
    return cam


def _custom(make):
    return lambda rt: make(_Aimed(aimed_camera(rt, LOOK_FROM[0])))


def _host(case, **kw):
    return lambda rt: scene_cases.build(rt, case, **kw)


# name -> (builder, samples per pixel of its cases, the first `of` views of an orbit for a host scene / None: LOOK_FROM)
SCENES = {
    "spheres300": (_custom(lambda cam: custom_scenes.many_spheres_scene(cam, 300)), 4, None),
    "spheres1200": (_custom(lambda cam: custom_scenes.many_spheres_scene(cam, 1200)), 4, None),
    "spheres6000": (_custom(lambda cam: custom_scenes.many_spheres_scene(cam, 6000)), 2, None),  # (the largest oracle job: a flat list)
    "media": (_custom(lambda cam: custom_scenes.media_scene(cam, 0)), 4, None),
    "tie": (_custom(lambda cam: custom_scenes.tie_scene(cam, 2)), 4, None),
    "materials65535": (_custom(lambda cam: custom_scenes.many_materials_scene(cam, 65533, depth=MAX_DEPTH)), 4, None),
    "textured_flat": (_custom(lambda cam: custom_scenes.textured_scene(cam, False)), 4, None),
    "textured_frames": (_custom(lambda cam: custom_scenes.textured_scene(cam, True)), 4, None),
    "cornell": (_host(CAMERA_CASE), 4, 30),
    "cornell_smoke": (_host("cornell_smoke_64x64_16spp", width=32), 4, 30),
    "two_perlin_spheres": (_host("two_perlin_spheres_80x45_8spp", width=40), 4, 12),
    "simple_light": (_host("simple_light_80x45_16spp", width=40), 4, 12),
    "earth": (_host("earth_ragged_image_80x45_8spp", width=40), 4, 12),
    "final_scene": (_host("c4_final_scene_64x64_8spp_d40", width=32, depth=MAX_DEPTH), 4, 12),
}


def scene(rt, name):
    if name not in _scenes:
        _scenes[name] = SCENES[name][0](rt)
        assert _scenes[name].camera.max_depth <= MAX_DEPTH, name
    return _scenes[name]


def spp_of(name):
    return SCENES[name][1]


def _scaled(v, k):
    return type(v)(v.x * k, v.y * k, v.z * k)


def three_views(rt, name, seed0):
    """Three views of the scene with different cameras and seeds seed0, seed0 + 1, seed0 + 2; the outer two with defocus (a lens of
    three pixel widths at the viewport where the scene's camera has none), the middle one without."""
    hs = scene(rt, name)
    of = SCENES[name][2]
    views = (rt.View * 3)()
    for k in range(3):
        if of is None:
            cam = aimed_camera(rt, LOOK_FROM[k])
            cam.samples_per_pixel, cam.max_depth, cam.background = hs.camera.samples_per_pixel, hs.camera.max_depth, hs.camera.background
        else:
            cam = rt.camera_look(hs, rt.orbit_look_from(hs, k, of))
        if k == 1:
            cam.defocus_angle = 0.0
        elif cam.defocus_angle <= 0.0:
            cam.defocus_angle = 0.6
            cam.defocus_disk_u, cam.defocus_disk_v = _scaled(cam.pixel_delta_u, 3.0), _scaled(cam.pixel_delta_v, -3.0)
        views[k].camera, views[k].seed = cam, seed0 + k
    assert len({bytes(views[k].camera) for k in range(3)}) == 3
    assert views[0].camera.defocus_angle > 0.0 and views[1].camera.defocus_angle == 0.0 and views[2].camera.defocus_angle > 0.0
    return views


def stress_list(n_pix, seed=7):
    """(list, listed pixels): a shuffled 60 % of the frame's pixels with 11 padding entries at random places; the length is made
    odd, so it is no multiple of 64"""
    g = np.random.default_rng(seed)
    chosen = g.choice(n_pix, size=(n_pix * 3) // 5, replace=False).astype(np.uint32)
    g.shuffle(chosen)
    pixels = np.insert(chosen, g.integers(0, chosen.size, 11), PAD)
    if pixels.size % 2 == 0:
        pixels = np.append(pixels, np.uint32(PAD))
    assert pixels.size % 64 != 0 and len(set(chosen.tolist())) == chosen.size
    return pixels.astype(np.uint32), chosen


def _k(features, lds, ordered, wide, aux, threads, ids_ok=1):
    return dict(features=FEAT[features], lds_level=lds, ordered=ordered, wide=wide, aux=aux, ids_ok=ids_ok, threads=threads)


OWN0, OWN1, REF = dict(walk="RT_WALK_OWN_TREES", wide=0), dict(walk="RT_WALK_OWN_TREES", wide=1), dict(walk="RT_WALK_REFERENCE_ORDER")

# id -> (scene, rt_scene_options fields, what rt_debug_last_kernel reports but for the job mode).  Workgroup threads: 1024 with the
# scene or its records in the LDS, 768 for the textures kernel in the reference's order, 256 without the LDS.  AUX (the small tables in
# the LDS) is on for every scene on the library's own trees whose tables fit 48 KiB — all but the 65 535 materials.  No scene reaches
# LDS level 2: scene creation never chooses it (rt_api.cpp: it measured slower than level 1).
CLASSES = {
    "spheres_solid-lds3-own-wide0": ("spheres300", OWN0, _k("spheres_solid", 3, 1, 0, 1, 1024)),
    "spheres_solid-lds3-own-wide1": ("spheres300", OWN1, _k("spheres_solid", 3, 1, 1, 1, 1024)),
    "spheres_solid-lds3-ref": ("spheres300", REF, _k("spheres_solid", 3, 0, 0, 0, 1024)),
    "quads_frames-lds3-own-wide0": ("cornell", OWN0, _k("quads_frames", 3, 1, 0, 1, 1024)),
    "quads_frames-lds3-own-wide1": ("cornell", OWN1, _k("quads_frames", 3, 1, 1, 1, 1024)),
    "quads_frames-lds3-ref": ("cornell", REF, _k("quads_frames", 3, 0, 0, 0, 1024)),
    "quads_frames_media-lds3-own": ("cornell_smoke", OWN0, _k("quads_frames_media", 3, 1, 0, 1, 1024)),
    "quads_frames_media-lds3-ref": ("cornell_smoke", REF, _k("quads_frames_media", 3, 0, 0, 0, 1024)),
    "textures-lds3-own-two_perlin_spheres": ("two_perlin_spheres", OWN0, _k("spheres_quads_textures", 3, 1, 0, 1, 1024)),
    "textures-lds3-own-simple_light": ("simple_light", OWN0, _k("spheres_quads_textures", 3, 1, 0, 1, 1024)),
    "textures-lds3-own-earth": ("earth", OWN0, _k("spheres_quads_textures", 3, 1, 0, 1, 1024)),
    "textures-lds3-ref-two_perlin_spheres": ("two_perlin_spheres", REF, _k("spheres_quads_textures", 3, 0, 0, 0, 768)),
    "textures-lds3-ref-simple_light": ("simple_light", REF, _k("spheres_quads_textures", 3, 0, 0, 0, 768)),
    "textures-lds3-ref-earth": ("earth", REF, _k("spheres_quads_textures", 3, 0, 0, 0, 768)),
    # (hand-made: images on quads, checkers of checkers, two Perlin tables, a textured light — custom_scenes.textured_scene)
    "textures-lds3-own-wide1-textured_flat": ("textured_flat", OWN1, _k("spheres_quads_textures", 3, 1, 1, 1, 1024)),
    "textures-lds3-ref-textured_flat": ("textured_flat", REF, _k("spheres_quads_textures", 3, 0, 0, 0, 768)),
    "all-lds3-own-media": ("media", OWN0, _k("all", 3, 1, 0, 1, 1024)),
    "all-lds3-ref-media": ("media", REF, _k("all", 3, 0, 0, 0, 1024)),
    "all-lds3-own-wide1-tie": ("tie", OWN1, _k("all", 3, 1, 1, 1, 1024)),
    "all-lds3-ref-tie": ("tie", REF, _k("all", 3, 0, 0, 0, 1024)),
    "all-lds3-own-wide1-textured_frames": ("textured_frames", OWN1, _k("all", 3, 1, 1, 1, 1024)),  # (textures inside frames and media)
    "all-lds1-own-wide0": ("spheres1200", OWN0, _k("all", 1, 1, 0, 1, 1024)),
    "all-lds1-own-wide1": ("spheres1200", OWN1, _k("all", 1, 1, 1, 1, 1024)),
    "all-lds1-ref": ("spheres6000", REF, _k("all", 1, 0, 0, 0, 1024)),  # (a flat list is few records in the reference's order: they fit)
    "all-lds0-own-wide0": ("spheres6000", OWN0, _k("all", 0, 1, 0, 1, 256)),
    "all-lds0-own-wide1": ("spheres6000", OWN1, _k("all", 0, 1, 1, 1, 256)),
    # (no scene the oracle can check is without the LDS in the reference's order by itself — that takes more than 4992 records, and
    # final_scene's BVH has 2819: the scene is forced out)
    "all-lds0-ref": ("spheres6000", dict(REF, use_lds=0), _k("all", 0, 0, 0, 0, 256)),
    "all-lds0-media-sequence": ("final_scene", OWN1, _k("all", 0, 1, 1, 1, 256)),
    "forced_out-cornell": ("cornell", dict(OWN0, use_lds=0), _k("all", 0, 1, 0, 1, 256)),
    "forced_out-simple_light": ("simple_light", dict(REF, use_lds=0), _k("all", 0, 0, 0, 0, 256)),
    "colour_parking-lds3-own": ("materials65535", OWN0, _k("spheres_quads_textures", 3, 1, 0, 0, 1024, ids_ok=0)),
}
FORCED_OUT = {"forced_out-cornell", "forced_out-simple_light", "all-lds0-ref"}  # scenes that fit the LDS (stats: lds_nodes > 0), rendered without it


def device_scene(rt, cls, **more):
    name, opts, _ = CLASSES[cls]
    opts = dict(opts, **more)
    opts["walk"] = getattr(rt, opts["walk"])
    return rt.DeviceScene(scene(rt, name), **opts)


def expected_kernel(cls, jobs):
    return dict(CLASSES[cls][2], jobs=jobs)


def check_stats(cls, stats):
    """DeviceScene.stats() against the class: the walk, and whether the scene (or its records) has an LDS image at all"""
    want = CLASSES[cls][2]
    assert stats["ordered"] == want["ordered"], (cls, stats)
    assert (stats["lds_nodes"] > 0) == (want["lds_level"] > 0 or cls in FORCED_OUT), (cls, stats)
