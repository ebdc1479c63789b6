"""GPU parity, bit for bit against the CPU oracle, on hand-made scenes with what only the nine stock scenes had so far: checker, noise
and image textures (on quads — the quad UV block of the shade stage —, inside Translate / RotateY frames, nested in checkers, as a
light's emission and a medium's albedo, images one texel wide or high, two Perlin tables and five images per scene) and spheres that
move in every direction (tests/custom_scenes.py: textured_scene, moving_scene, many_spheres_scene(textured=True),
random_scene(textures=True)).  tests/test_textured_scene_conditions.py holds, on the oracle alone, that these scenes do evaluate their
textures where a camera ray sees them.

Every frame is 37x37 at 2 to 4 samples and depth <= 8, seen through kernel_classes.aimed_camera."""
import numpy as np
import pytest

import albedo_helpers
import custom_scenes
import guided_helpers
import kernel_classes
from test_gpu_ties import WALKS, bits, check

pytestmark = pytest.mark.gpu


def aimed(rt):
    return kernel_classes._Aimed(kernel_classes.aimed_camera(rt, kernel_classes.LOOK_FROM[0]))


def assert_same(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} values differ, first at {bad[:4]}"


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("frames", [False, True])
def test_textured_scene_in_every_walk(rt, oracle, gpu, frames, order):
    check(rt, oracle, custom_scenes.textured_scene(aimed(rt), frames, order), f"textured scene, frames={frames}, order {order}")


@pytest.mark.parametrize("n, frames", [(40, True), (3, False)])
def test_moving_scene_in_every_walk(rt, oracle, gpu, n, frames):
    check(rt, oracle, custom_scenes.moving_scene(aimed(rt), n=n, frames=frames), f"moving scene, n={n}, frames={frames}")


@pytest.mark.parametrize("name", ["textured_frames", "moving"])
def test_counters_match_the_oracle_in_tight_mode(rt, oracle, gpu, name):
    """as test_gpu_parity's test of this name: the same rays, draws, noise evaluations and image lookups in both walks"""
    import torch
    scene = custom_scenes.textured_scene(aimed(rt), True) if name == "textured_frames" else custom_scenes.moving_scene(aimed(rt))
    params = rt.render_params(seed=4)
    want_img, want = oracle.render(scene, params, aabb_mode=oracle.ORC_AABB_TIGHT, want_counters=True)
    assert (want["noise_evals"] > 0 and want["image_lookups"] > 0) == (name == "textured_frames")
    for ordered in (0, 2):
        ds = rt.DeviceScene(scene, walk=rt.RT_WALK_OWN_TREES if ordered else rt.RT_WALK_REFERENCE_ORDER)
        assert ds.stats()["ordered"] == (1 if ordered else 0)
        d = torch.zeros(scene.width * scene.height * 3, dtype=torch.float64, device="cuda")
        got = ds.render_device_counted(params, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert_same(d.cpu().numpy(), want_img, f"{name}, ordered={ordered}")
        for key in ("samples", "rays", "rng_draws", "noise_evals", "image_lookups"):
            assert got[key] == want[key], (name, ordered, key, got[key], want[key])


@pytest.mark.parametrize("n,level", [(300, 3), (1200, 1), (6000, 0)])
def test_textured_spheres_at_every_lds_level_in_both_record_forms(rt, oracle, gpu, n, level):
    """test_gpu_ties' test_scenes_at_every_lds_level_in_both_record_forms with textured materials and moving spheres among the n: the
    texture code of the every-feature kernels at LDS levels 1 and 0, and the postponement of noise hits where they are scattered among
    other lanes' hits"""
    scene = custom_scenes.many_spheres_scene(aimed(rt), n, textured=True)
    params = rt.render_params(seed=3, sample_end=2 if n == 6000 else 0)
    want = oracle.render(scene, params)
    for opts in (dict(walk=rt.RT_WALK_OWN_TREES, wide=0), dict(walk=rt.RT_WALK_OWN_TREES, wide=1), dict(walk=rt.RT_WALK_REFERENCE_ORDER)):
        ds = rt.DeviceScene(scene, **opts)
        if opts.get("wide") == 1:
            assert rt.debug_last_launch is not None and (ds.stats()["lds_nodes"] > 0) == (level > 0), ds.stats()
        got = ds.render(params)
        assert_same(got, want, (n, opts))
        if opts.get("wide") == 1:
            assert rt.debug_last_launch()["lds_level"] == level, rt.debug_last_launch()


@pytest.mark.parametrize("shortcuts", [(0, 0, 0, 0, 1, 0, 1, 0), (8, 0, 1, 1, 64, 3, 0, 1), (0, 1, 0, 1, 2, 1000, 1, 0), (3, 1, 1, 0, 4, 32, 1, 1), (8, 1, 1, 1, 4, 32, 0, 0),
                                       (8, 1, 1, 0, 4, 32, 1, 0)])
def test_walk_shortcuts_never_change_the_textured_image(rt, oracle, gpu, shortcuts):
    """the option combinations of test_gpu_ties' test_walk_shortcuts_never_change_the_image, on a scene whose noise hits are scattered
    among other lanes' hits (there: one big noise sphere)"""
    scene = custom_scenes.textured_scene(aimed(rt), True)
    params = rt.render_params(seed=3)
    want = oracle.render(scene, params)
    flat_max, start_shortcut, defer_instances, seq_lookahead, slow_min, slow_age, quad_filter, medium_first = shortcuts
    got = rt.DeviceScene(scene, flat_max=flat_max, start_shortcut=start_shortcut, defer_instances=defer_instances, seq_lookahead=seq_lookahead,
                         slow_min=slow_min, slow_age=slow_age, quad_filter=quad_filter, medium_first=medium_first).render(params)
    assert_same(got, want, f"textured scene, shortcuts {shortcuts}")


def test_random_textured_object_graphs(rt, oracle, gpu):
    """Fuzz: random_scene(textures=True), seeds 0..19, in the three variants of test_gpu_ties' test_random_object_graphs.  Textures and
    motion do not decide whether a graph gets the library's own trees: each seed is ordered iff the plain scene of that seed is."""
    cam = aimed(rt)
    params = rt.render_params(seed=5)
    for seed in range(20):
        scene = custom_scenes.random_scene(cam, seed, textures=True)
        plain_ordered = rt.DeviceScene(custom_scenes.random_scene(cam, seed), walk=rt.RT_WALK_OWN_TREES).stats()["ordered"]
        want = oracle.render(scene, params)
        for ordered in (2, 3, 0):  # (3: own trees with four children per record)
            ds = rt.DeviceScene(scene, walk=getattr(rt, WALKS[min(ordered, 2)]), wide=1 if ordered == 3 else 0)
            assert ds.stats()["ordered"] == (plain_ordered if ordered else 0), (seed, ordered)
            assert_same(ds.render(params), want, f"random textured scene {seed}, variant {ordered}, ordered={ds.stats()['ordered']}")


@pytest.mark.parametrize("walk", ["RT_WALK_OWN_TREES", "RT_WALK_REFERENCE_ORDER"])
def test_the_albedo_and_surface_id_scenes_of_the_textured_scene(rt, oracle, gpu, walk):
    """rt_scene_create_albedo under rt.albedo_camera against the oracle's render of the rule-applied description (albedo_helpers), and
    rt_scene_create_surface_ids against the oracle's render of the description that rt.surface_id_tables yields"""
    scene = custom_scenes.textured_scene(aimed(rt), True)
    params = rt.render_params(seed=3)
    rule = albedo_helpers.AlbedoScene(rt, scene)
    white = rt.albedo_camera(scene.camera)
    assert bytes(white) == bytes(rule.camera)
    got = rt.DeviceScene(scene, albedo=True, walk=getattr(rt, walk)).render(params, camera=white)
    assert_same(got, oracle.render(rule, params), f"albedo scene, {walk}")
    ids = guided_helpers.SurfaceIdScene(rt, scene)
    for ours, theirs in zip((ids._spheres, ids._quads, ids._media, ids._materials, ids._textures), rt.surface_id_tables(scene)):
        assert bytes(ours) == bytes(theirs), "rt_surface_id_tables against the rule in Python (guided_helpers.id_rule)"
    black = rt.surface_id_camera(scene.camera)
    got = rt.DeviceScene(scene, surface_ids=True, walk=getattr(rt, walk)).render(params, camera=black)
    assert_same(got, oracle.render(ids, params, camera=black), f"surface-ID scene, {walk}")
