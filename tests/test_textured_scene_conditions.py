"""What the hand-made textured and moving scenes (custom_scenes.textured_scene, moving_scene, many_spheres_scene(textured=True)) must
show for the GPU tests built on them (test_gpu_textured_scenes.py) to mean anything — checked on the CPU oracle alone: the textures are
really evaluated, every image and either Perlin table is read on a surface that a camera ray hits first, and the motion changes the
frame."""
import ctypes as C

import numpy as np
import pytest

import albedo_helpers
import custom_scenes
import kernel_classes


def aimed(rt, k=0):
    return kernel_classes._Aimed(kernel_classes.aimed_camera(rt, kernel_classes.LOOK_FROM[k]))


SCENES = {
    "textured_flat": lambda cam: custom_scenes.textured_scene(cam, False),
    "textured_frames": lambda cam: custom_scenes.textured_scene(cam, True),
    "many_spheres_300_textured": lambda cam: custom_scenes.many_spheres_scene(cam, 300, textured=True),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_the_oracle_evaluates_noise_and_images(rt, oracle, name):
    scene = SCENES[name](aimed(rt))
    _, counters = oracle.render(scene, rt.render_params(seed=3), want_counters=True)
    assert counters["noise_evals"] > 0 and counters["image_lookups"] > 0 and counters["rng_draws"] > 0, counters
    assert counters["samples"] == scene.width * scene.height * scene.camera.samples_per_pixel


@pytest.mark.parametrize("name", list(SCENES))
def test_every_image_and_perlin_table_is_seen_by_a_camera_ray(rt, oracle, name):
    """One sample per pixel of the scene under the albedo rule (every material a light of its own texture) is the colour of the first
    surface hit.  An image is seen if one of its texels' colours is a pixel; a Perlin table, whose greys carry no mark of the table,
    if putting another table in its place changes a pixel."""
    scene = SCENES[name](aimed(rt))
    d = scene.desc
    assert d.n_images >= 1 and d.n_perlins == 2
    first = albedo_helpers.AlbedoScene(rt, scene)
    params = rt.render_params(seed=3, sample_end=1)
    frame = oracle.render(first, params).reshape(-1, 3)
    pixels = {tuple(p) for p in frame}
    for k in range(d.n_images):
        im = d.images[k]
        texels = np.ctypeslib.as_array(im.rgb, shape=(im.height * im.width, 3))
        colours = {tuple((float(c) / 255.0) ** 2.2 for c in t) for t in texels if t.any()}
        assert colours & pixels, f"{name}: no camera ray sees image {k} ({im.width}x{im.height})"
    if name.startswith("textured"):
        assert (0.0, 0.0, 0.0) in pixels and any(1.0 in p for p in pixels)  # the zero region and the byte 255 of the 8x8 image
    for k in range(d.n_perlins):
        tables = (rt.Perlin * d.n_perlins)(*[rt.Perlin.from_buffer_copy(d.perlins[i]) for i in range(d.n_perlins)])
        tables[k] = custom_scenes.perlin_table_b(77 + k)
        first.desc.perlins = tables
        other = oracle.render(first, params).reshape(-1, 3)
        first.desc.perlins = d.perlins
        assert (other != frame).any(), f"{name}: no camera ray sees a noise texture of Perlin table {k}"


def test_the_textured_scene_is_what_it_says(rt):
    """five images of the five sizes, each read by a material; the flat form is spheres, quads and one list"""
    for frames in (False, True):
        d = custom_scenes.textured_scene(aimed(rt), frames).desc
        assert [(d.images[k].width, d.images[k].height) for k in range(d.n_images)] == custom_scenes.IMAGE_SIZES
        used = set()

        def reach(t):
            x = d.textures[t]
            if x.kind == rt.RT_TEXTURE_IMAGE:
                used.add(("image", x.image))
            elif x.kind == rt.RT_TEXTURE_NOISE:
                used.add(("perlin", x.perlin))
            elif x.kind == rt.RT_TEXTURE_CHECKER:
                reach(x.even); reach(x.odd)

        materials_in_use = {d.spheres[i].material for i in range(d.n_spheres)} | {d.quads[i].material for i in range(d.n_quads)} | \
                           {d.media[i].phase_material for i in range(d.n_media)}
        for m in materials_in_use:
            if d.materials[m].texture >= 0:
                reach(d.materials[m].texture)
        assert used == {("image", k) for k in range(5)} | {("perlin", 0), ("perlin", 1)}
        assert (d.n_translates, d.n_rotates, d.n_media) == ((3, 3, 2) if frames else (0, 0, 0))  # (two frames, a third inside one)
        assert (frames or d.n_lists == 1) and d.n_bvhs == 0
        octants = {tuple(np.sign(d.spheres[i].center.tuple()).astype(int)) for i in range(d.n_spheres)}
        assert len(octants) >= 6  # (the other two, (-, -, -) and (+, +, -), hold the floor, the back quad and the skewed quad)


def test_motion_changes_the_moving_scene(rt, oracle):
    """against the same scene with every sphere left at its time-0 place: more than a tenth of the pixels differ"""
    for n, frames in ((40, True), (3, False)):
        scene = custom_scenes.moving_scene(aimed(rt), n=n, frames=frames)
        still = custom_scenes.without_motion(scene)
        assert sum(scene.desc.spheres[i].is_moving for i in range(scene.desc.n_spheres)) > 0
        assert not any(still.desc.spheres[i].is_moving for i in range(still.desc.n_spheres))
        params = rt.render_params(seed=3)
        a, b = oracle.render(scene, params).reshape(-1, 3), oracle.render(still, params).reshape(-1, 3)
        differ = (a != b).any(axis=1).mean()
        assert differ > 0.1, (n, frames, differ)


def test_the_second_generator_leaves_the_first_alone(rt):
    """random_scene(textures=True) and many_spheres_scene(textured=True) are the plain scenes' object graphs: the same spheres at time 0,
    the same quads up to their materials, the same frames and media"""
    cam = aimed(rt)

    def geometry(scene):
        d = scene.desc
        return ([(d.spheres[i].center.tuple(), d.spheres[i].radius) for i in range(d.n_spheres)],
                [(d.quads[i].q.tuple(), d.quads[i].u.tuple(), d.quads[i].v.tuple()) for i in range(d.n_quads)],
                albedo_helpers.table_bytes(d.lists, d.n_lists), albedo_helpers.table_bytes(d.list_items, d.n_list_items),
                albedo_helpers.table_bytes(d.translates, d.n_translates), albedo_helpers.table_bytes(d.rotates, d.n_rotates),
                [(bytes(d.media[i].boundary), d.media[i].neg_inv_density) for i in range(d.n_media)], bytes(d.world))

    moving = textured = 0
    for seed in range(20):
        plain, tex = custom_scenes.random_scene(cam, seed), custom_scenes.random_scene(cam, seed, textures=True)
        assert geometry(plain) == geometry(tex), seed
        assert bytes(plain.camera) == bytes(tex.camera)
        moving += sum(tex.desc.spheres[i].is_moving for i in range(tex.desc.n_spheres))
        textured += tex.desc.n_images + tex.desc.n_perlins
    assert moving > 0 and textured == 20 * 4  # (some sphere moves; two images and two Perlin tables per scene)
    plain, tex = custom_scenes.many_spheres_scene(cam, 300), custom_scenes.many_spheres_scene(cam, 300, textured=True)
    assert geometry(plain) == geometry(tex)
    d = tex.desc
    assert sum(d.spheres[i].is_moving for i in range(d.n_spheres)) == 60
    used = {d.spheres[i].material for i in range(d.n_spheres)}
    textured = {m for m in used if d.materials[m].texture >= 0 and d.textures[d.materials[m].texture].kind != rt.RT_TEXTURE_SOLID}
    assert len(textured) == 5 and len(used) == 16  # six of the 17 materials (every third) gave way to the five textured ones
