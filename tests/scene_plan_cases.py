"""Shared by tests/test_scene_plan.py and tests/test_gpu_scene_plan.py (not a test module): the scenes and option sets whose plan
(rt_debug_scene_plan) is pinned in tests/golden/scene_plan_pins.json, and the key of a case in that file.

The pins were recorded from the library BEFORE scene creation was split into plan and upload: that rt_scene_create_ex, with a patch
that made `upload` hash its vector instead of copying it and skipped the device checks, run over every case below."""
import json
from pathlib import Path

import custom_scenes
import kernel_classes as kc
import scene_cases

PINS = Path(__file__).resolve().parent / "golden" / "scene_plan_pins.json"

# the three walks a scene can be given (rt_scene_options): the reference's order, own trees with two- and with four-child records
OPTION_SETS = {"ref": kc.REF, "own-wide0": kc.OWN0, "own-wide1": kc.OWN1}

STOCK = ["random_balls", "two_spheres", "earth", "two_perlin_spheres", "quads", "simple_light", "cornell_box", "cornell_smoke", "final_scene"]


def _stock(index, width):
    return lambda rt: rt.HostScene(index, width=width, spp=1, depth=4, earth_image=scene_cases.EARTH_SMALL)


def _custom(make):
    return lambda rt: make(kc._Aimed(kc.aimed_camera(rt, kc.LOOK_FROM[0])))


HAND_MADE = {
    "spheres300": _custom(lambda cam: custom_scenes.many_spheres_scene(cam, 300)),
    "spheres1200": _custom(lambda cam: custom_scenes.many_spheres_scene(cam, 1200)),
    "spheres6000": _custom(lambda cam: custom_scenes.many_spheres_scene(cam, 6000)),
    "spheres300_textured": _custom(lambda cam: custom_scenes.many_spheres_scene(cam, 300, textured=True)),
    "tie": _custom(lambda cam: custom_scenes.tie_scene(cam, 2)),
    "single_sphere": _custom(custom_scenes.single_sphere_scene),
    "empty_frame": _custom(custom_scenes.empty_frame_scene),
    "media": _custom(lambda cam: custom_scenes.media_scene(cam, 0)),
    "media_nested": _custom(lambda cam: custom_scenes.media_scene(cam, 1, nested=True)),
    "nested_frames": _custom(custom_scenes.nested_frames_scene),
    "many_media": _custom(custom_scenes.many_media_scene),
    "instances20": _custom(lambda cam: custom_scenes.many_instances_scene(cam, 20)),
    "instances40_quads": _custom(lambda cam: custom_scenes.many_instances_scene(cam, 40, spheres=False)),
    "materials65535": _custom(lambda cam: custom_scenes.many_materials_scene(cam, 65533)),
    "textured_flat": _custom(lambda cam: custom_scenes.textured_scene(cam, False)),
    "textured_frames": _custom(lambda cam: custom_scenes.textured_scene(cam, True)),
    "moving": _custom(custom_scenes.moving_scene),
    "random7_textures": _custom(lambda cam: custom_scenes.random_scene(cam, 7, textures=True)),
}

SCENES = dict({name: _stock(k, 64) for k, name in enumerate(STOCK)}, **HAND_MADE)
_built = {}


def scene(rt, name, width=None):
    """the scene of a pinned case; `width`: a stock scene at another image_width (the plan does not depend on it)"""
    key = (name, width)
    if key not in _built:
        _built[key] = SCENES[name](rt) if width is None else _stock(STOCK.index(name), width)(rt)
    return _built[key]


def options(rt, option_set, **more):
    opts = dict(OPTION_SETS[option_set], **more)
    opts["walk"] = getattr(rt, opts["walk"])
    return opts


def cases():
    return [(name, option_set) for name in SCENES for option_set in OPTION_SETS]


def key(name, option_set):
    return f"{name}/{option_set}"


def pins():
    return json.loads(PINS.read_text())
