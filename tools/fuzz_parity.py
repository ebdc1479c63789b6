#!/usr/bin/env python3
"""Long fuzz run of tests/custom_scenes.py::random_scene: GPU (the reference-order walk, the library's own trees with two and with
four children per record, with the default and with odd settings of the walk's shortcuts) against the oracle, bit for bit.
start_inline (the start sphere's test where a query begins, or in the sphere stage) is drawn per scene, for all four forms.

random_scene mixes quads, frames and media into nearly every graph, so its renders seldom run a spheres-only kernel whose start leaf
is one sphere — the only place the inline start test is compiled.  Every eighth seed therefore renders a ground graph as well
(ground_graph below: spheres only, one big sphere under 1-90 small ones, the camera outside, inside or on it), with start_inline 1
and 0.  The last line counts, per family, the renders that really ran the inline test (rt_debug_last_start, rt_debug_last_kernel).
A third family, "textured": random_scene(..., textures=True) — the same graphs with checker, noise and image textures (on Lambertians,
lights and media) and moving spheres, rendered from a camera turned towards them.
Usage: python tools/fuzz_parity.py [first_seed] [count]"""
import importlib, random, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
rt = importlib.import_module("rust-tracing_amd")
import custom_scenes, scene_cases, oracle_lib

first, count = (int(sys.argv[1]) if len(sys.argv) > 1 else 0), (int(sys.argv[2]) if len(sys.argv) > 2 else 500)
cam = scene_cases.build(rt, "ragged_cornell_37x37_4spp")


class _Aimed:
    def __init__(self, camera):
        self.camera = camera


def ground_graph(seed):
    """Spheres only: a big ground sphere (top at y = 0; it moves in two graphs of five) under small ones that rest on it, float, sink
    into it or lie inside it, a lamp inside the ground, now and then an exact copy of the ground (ties).  The camera is outside,
    inside the ground, exactly on its surface or just above it.  1-90 small spheres: two- and four-child records."""
    rnd = random.Random(seed ^ 0x5eed)
    radius = rnd.choice([30.0, 100.0, 1000.0])
    where = rnd.choice(["outside", "outside", "inside", "on_surface", "grazing"])
    look_from = {"outside": (rnd.uniform(-8, 8), rnd.uniform(0.3, 4.0), rnd.uniform(5, 10)), "inside": (rnd.uniform(-4, 4), -rnd.uniform(0.5, radius / 4), rnd.uniform(3, 9)),
                 "on_surface": (0.0, 0.0, 0.0), "grazing": (0.0, rnd.choice([0.0005, 0.001, 0.002]), 4.0)}[where]
    look_at = (rnd.uniform(-1, 1), rnd.uniform(-1.5, 0.5), rnd.uniform(-5, 0))
    camera = rt.camera_look(cam, look_from, look_at)
    if where in ("on_surface", "grazing") or rnd.random() < 0.5:
        camera.defocus_angle = 0.0  # every ray starts at look_from exactly
    s = custom_scenes.CustomScene(_Aimed(camera), spp=2, depth=6, background=(0.7, 0.8, 1.0) if rnd.random() < 0.7 else (0.0, 0.0, 0.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(4)]
    mats += [s.metal(rnd.random(), rnd.random(), rnd.random(), rnd.choice([0.0, 0.3, 1.5])), s.dielectric(rnd.choice([1.5, 1.0 / 1.5, 2.4])),
             s.light(rnd.uniform(1, 8), rnd.uniform(1, 8), rnd.uniform(1, 8))]
    items = [s.sphere((0.0, -radius, 0.0), radius, rnd.choice(mats))]
    if rnd.random() < 0.4:
        s.spheres[0].center_vec, s.spheres[0].is_moving = rt.Vec3(rnd.uniform(-0.2, 0.2), rnd.uniform(-0.5, 0.5), 0.0), 1
    items.append(s.sphere((rnd.uniform(-2, 2), -rnd.uniform(3.0, 8.0), rnd.uniform(0, 4)), rnd.uniform(0.5, 2.5), mats[6]))  # a lamp inside the ground
    for _ in range(rnd.choice([1, 5, 20, 62, 70, 90])):
        r = rnd.uniform(0.1, 0.6)
        y = rnd.choice([r, r, r + rnd.uniform(0.0, 1.5), rnd.uniform(-r, r), -rnd.uniform(1.0, 6.0)])  # tangent | floating | sunk | inside
        items.append(s.sphere((rnd.uniform(-5, 5), y, rnd.uniform(-5, 5)), r, rnd.choice(mats)))
    if rnd.random() < 0.15:
        items.insert(rnd.randint(1, len(items)), s.sphere((0.0, -radius, 0.0), radius, rnd.choice(mats)))
    return s.finish(s.list(items))


bad, renders, inline_renders = 0, {"random": 0, "ground": 0, "textured": 0}, {"random": 0, "ground": 0, "textured": 0}
aimed = _Aimed(rt.camera_look(cam, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0)))


def check(family, scene, seed, start_inline):
    global bad
    rt.amd_lib().rt_debug_set_start_inline(start_inline)
    for render_seed in (5, 6):
        params = rt.render_params(seed=render_seed)
        want = oracle_lib.render(scene, params)
        variants = [dict(walk=rt.RT_WALK_REFERENCE_ORDER), dict(walk=rt.RT_WALK_OWN_TREES, wide=0), dict(walk=rt.RT_WALK_OWN_TREES, wide=1),
                    dict(walk=rt.RT_WALK_OWN_TREES, wide=1, flat_max=seed % 9, leaf_max=1 + seed % 8, start_shortcut=seed % 2, defer_instances=(seed >> 1) % 2,
                         seq_lookahead=(seed >> 2) % 2, slow_min=1 + seed % 5, slow_age=seed % 40, quad_filter=(seed >> 3) % 2, medium_first=(seed >> 4) % 2)]
        for opts in variants:
            got = rt.DeviceScene(scene, **opts).render(params)
            renders[family] += 1
            inline_renders[family] += rt.debug_last_start()["ran_inline"]
            if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
                bad += 1
                print("MISMATCH", family, "scene", seed, "start_inline", start_inline, "render seed", render_seed, opts, int((got.view(np.uint64) != want.view(np.uint64)).sum()), "values", flush=True)


for seed in range(first, first + count):
    check("random", custom_scenes.random_scene(cam, seed), seed, (seed >> 5) % 2)
    check("textured", custom_scenes.random_scene(aimed, seed, textures=True), seed, (seed >> 5) % 2)
    if seed % 8 == 3:
        ground = ground_graph(seed)
        for value in (1, 0):
            check("ground", ground, seed, value)
    if seed % 100 == 99:
        print("...", seed + 1 - first, "scenes,", bad, "mismatches", flush=True)
print("done:", count, "scenes,", bad, "mismatches;", "renders that ran the inline start test:",
      ", ".join(f"{inline_renders[f]} of {renders[f]} ({f} graphs)" for f in renders))
sys.exit(1 if bad else 0)
