"""Where the ordered walk's box round leaves work to later stages (rt_kernel.hip): a lane that goes on to a leaf keeps the leaf's PACKED
reference and its primitive stage takes it apart (o_next; the sphere stage steps index and count in place, one sphere per round; the
quad stage decodes once; the start shortcuts hand the same packed form over).  The cases on the stack's depth and on the choice among a
record's four children pin what two further changes of the box round would touch (the stack position carried as an address; one
reference read after the choice) — both were measured and not kept, the cases stay for whoever tries again.

Every frame here is held to the CPU oracle bit for bit (u64 views of the f64 sums).  Frames are at most 40x24 at 2-4 samples, depth 8.

What a case stands on is checked from the compiled scene, not assumed: the leaf counts from the scene compiler's records
(debug_wide_records / debug_ordered_layout), the kernel that ran from debug_last_kernel, the stack bound from stats().  The visit
statistics of a counted render (debug_visit_stats) count visits by how many children were left and what the walk went on with, not by
slot; that every slot of the four-sphere record is chosen is shown by the frame instead: each of the four spheres is a lamp of its own
colour on a black background, a pixel of that colour is a camera ray whose walk went on with that child, and the oracle frame has
pixels of all four."""
import math
import os

import numpy as np
import pytest

import custom_scenes
import kernel_classes as kc
import scene_cases
from adaptive_helpers import SENTINEL, assert_bits, bits

pytestmark = pytest.mark.gpu

DEPTH = 8
OREF_KIND_SHIFT, OREF_COUNT_SHIFT, OREF_COUNT_MASK, OREF_INDEX_MASK = 29, 26, 7, (1 << 26) - 1  # rt_layout.h
OK_SPHERES, OK_QUADS = 1, 2
OREF_MAX_LEAF = 8
SPHERES_WIDE = dict(lds_level=3, ordered=1, wide=1, aux=1, jobs=0, ids_ok=1, threads=1024)
_base = {}


class _Aimed:
    def __init__(self, camera):
        self.camera = camera


def base_scene(rt, w, h):
    """random-spheres at w x h: scene 0 itself, and the camera the hand-made scenes here are seen through"""
    if (w, h) not in _base:
        hs = rt.HostScene(0, width=w, aspect=w / h, spp=4, depth=DEPTH)
        assert (hs.width, hs.height) == (w, h)
        _base[(w, h)] = hs
    return _base[(w, h)]


def look(rt, w, h, look_from, look_at, spp):
    cam = rt.camera_look(base_scene(rt, w, h), look_from, look_at)
    cam.samples_per_pixel, cam.max_depth, cam.defocus_angle = spp, DEPTH, 0.0  # every camera ray starts at look_from exactly
    return cam


def leaf_counts(refs, kind):
    refs = np.asarray(refs, dtype=np.uint32).reshape(-1)
    leaves = refs[(refs >> OREF_KIND_SHIFT) == kind]
    return ((leaves >> OREF_COUNT_SHIFT) & OREF_COUNT_MASK) + 1, leaves & OREF_INDEX_MASK


# ---- A: sphere leaves of several spheres, stepped across rounds ---------------------------------------------------------------------
def clusters_scene(rt, k, n_min):
    """clusters of k spheres of radius 0.5 whose centres lie on a small ring (radius 0.15; 0.08 for the largest leaf), over a ground
    sphere, at least n_min primitives in all: spheres that overlap this much are dearer to split than to test one after the other, so
    the scene compiler keeps a cluster in one leaf; each sphere sticks out of the others on its own side, and the cluster's box has
    empty corners.  Seen from close by, so that a pixel is a tenth of a unit."""
    cam = look(rt, 32, 24, (-4.0, 1.0, 6.5), (-4.0, 0.6, 3.0), 4)
    s = custom_scenes.CustomScene(_Aimed(cam), spp=4, depth=DEPTH, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(0.8, 0.3, 0.3), s.lambertian(0.3, 0.8, 0.3), s.metal(0.8, 0.8, 0.9, 0.0), s.dielectric(1.5), s.light(3, 3, 3)]
    items = [s.sphere((0.0, -1000.0, 0.0), 1000.0, s.lambertian(0.5, 0.5, 0.5))]
    ring = 0.08 if k == OREF_MAX_LEAF else 0.15
    c = 0
    while len(items) < n_min:
        x0, z0 = -4.5 + 3.0 * (c % 4), 3.0 - 2.0 * (c // 4)
        for j in range(k):
            a = 2.0 * math.pi * j / k
            items.append(s.sphere((x0 + ring * math.cos(a), 0.5 + 0.8 * (c % 2) + ring * math.sin(a), z0), 0.5, mats[(c + j) % len(mats)]))
        c += 1
    return s.finish(s.list(items))


def pixel_rays(cam):
    """origin (3,) and directions (h, w, 3) of the rays through the pixel centres"""
    v = lambda a: np.array([a.x, a.y, a.z])
    ys, xs = np.mgrid[0:cam.image_height, 0:cam.image_width]
    d = v(cam.pixel00_loc) + xs[..., None] * v(cam.pixel_delta_u) + ys[..., None] * v(cam.pixel_delta_v) - v(cam.center)
    return v(cam.center), d


def first_hits(origin, d, centers, radii):
    """t of the first intersection of every ray with every sphere (inf: none), shape (h, w, n)"""
    oc = origin - centers  # (n, 3)
    a = (d * d).sum(-1)[..., None]
    hb = np.einsum("hwk,nk->hwn", d, oc)
    c = (oc * oc).sum(-1) - radii * radii
    disc = hb * hb - a * c
    t = (-hb - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
    return np.where((disc >= 0) & (t > 0.001), t, np.inf)


@pytest.mark.parametrize("leaf_max,n_min", [(2, 70), (3, 70), (OREF_MAX_LEAF, 70), (3, 8)])
def test_sphere_leaves_of_several_spheres_are_stepped_across_rounds(rt, oracle, gpu, leaf_max, n_min):
    """70 primitives and more: four-child records; 10: the two-child kernel (visit_record)"""
    hs = clusters_scene(rt, leaf_max, n_min)
    wide = n_min == 70
    if wide:
        rec = rt.debug_wide_records(hs, leaf_max=leaf_max, flat_max=0)
        assert rec["wide"]
        refs = rec["refs"]
    else:
        lay = rt.debug_ordered_layout(hs, leaf_max=leaf_max, flat_max=0)
        assert lay["ordered"]
        refs = lay["nodes"][:, 12:14]
    counts, first = leaf_counts(refs, OK_SPHERES)
    if counts.size == 0 or counts.max() != leaf_max:
        pytest.skip(f"the scene compiler made no sphere leaf of {leaf_max}: counts {sorted(set(counts.tolist()))}")
    # a leaf of the largest count whose LAST sphere alone is hit by some pixel's ray, and a ray through its box that hits none of it
    o, d = pixel_rays(hs.camera)
    lay = rt.debug_ordered_layout(hs, leaf_max=leaf_max, flat_max=0)
    sp = lay["spheres"]
    t = first_hits(o, d, sp[:, 0:3], sp[:, 3])
    last_only = box_miss = False
    for cnt, f in zip(counts.tolist(), first.tolist()):
        if cnt != leaf_max:
            continue
        tl = t[..., f:f + cnt]
        hit = np.isfinite(tl)
        last_only |= bool((hit[..., -1] & ~hit[..., :-1].any(-1)).any())
        lo = (sp[f:f + cnt, 0:3] - sp[f:f + cnt, 3:4]).min(0)
        hi = (sp[f:f + cnt, 0:3] + sp[f:f + cnt, 3:4]).max(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / d, (hi - o) / d
        enter, leave = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
        box_miss |= bool(((enter < leave) & (leave > 0.001) & ~hit.any(-1)).any())
    assert last_only and box_miss, (last_only, box_miss)
    params = rt.render_params(seed=21)
    want = oracle.render(hs, params)
    ds = rt.DeviceScene(hs, leaf_max=leaf_max, flat_max=0)
    got = ds.render(params)
    assert rt.debug_last_kernel() == dict(SPHERES_WIDE, features=rt.RT_FEAT_SPHERES_SOLID, wide=1 if wide else 0)
    assert_bits(got, want, f"sphere leaves of up to {leaf_max}, {'four' if wide else 'two'}-child records")


# ---- A: quad leaves (the filter path: count 6; count 1) -----------------------------------------------------------------------------
def test_cornell_quad_leaves_through_the_filter(rt, oracle, gpu):
    hs = scene_cases.build(rt, "c3_cornell_box_64x64_16spp_d50", width=24, spp=4, depth=DEPTH)
    assert (hs.width, hs.height) == (24, 24)
    counts, _ = leaf_counts(rt.debug_ordered_layout(hs)["nodes"][:, 12:14], OK_QUADS)
    assert counts.max() >= 6, counts
    params = rt.render_params(seed=3)
    assert_bits(rt.DeviceScene(hs).render(params), oracle.render(hs, params), "Cornell 24x24")
    assert rt.debug_last_kernel()["features"] == rt.RT_FEAT_QUADS_FRAMES


def test_a_scene_of_one_quad(rt, oracle, gpu):
    cam = look(rt, 24, 24, (0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 4)
    s = custom_scenes.CustomScene(_Aimed(cam), spp=4, depth=DEPTH, background=(0.7, 0.8, 1.0))
    hs = s.finish(s.quad((-2, -1.5, 0), (4, 0, 0), (0, 3, 0), s.metal(0.8, 0.6, 0.4, 0.1)))
    params = rt.render_params(seed=4)
    assert_bits(rt.DeviceScene(hs).render(params), oracle.render(hs, params), "one quad")


# ---- A: the start shortcut hands the packed form over ---------------------------------------------------------------------------------
class inline:
    def __init__(self, rt, value):
        self.rt, self.value = rt, value

    def __enter__(self):
        assert self.rt.amd_lib().rt_debug_set_start_inline(self.value) == 0

    def __exit__(self, *exc):
        self.rt.amd_lib().rt_debug_set_start_inline(int(os.environ.get("RT_START_INLINE", "1")))


def test_two_spheres_start_with_a_leaf_of_two(rt, oracle, gpu):
    hs = scene_cases.build(rt, "two_spheres_80x45_8spp", width=40, spp=4, depth=DEPTH)
    params = rt.render_params(seed=6)
    want = oracle.render(hs, params)
    got = rt.DeviceScene(hs).render(params)
    start = rt.debug_last_start()
    assert start["stage"] == 1 and start["end"] > start["first"] + 1 and start["ran_inline"] == 0, start
    assert_bits(got, want, "two_spheres: the start leaf's spheres in the sphere stage")


@pytest.mark.parametrize("value", [1, 0])
def test_random_spheres_start_leaf_inline_and_in_the_stage(rt, oracle, gpu, value):
    hs = base_scene(rt, 40, 24)
    params = rt.render_params(seed=5)
    ds = rt.DeviceScene(hs)
    with inline(rt, value):
        got = ds.render(params)
    assert rt.debug_last_kernel() == dict(SPHERES_WIDE, features=rt.RT_FEAT_SPHERES_SOLID)
    assert rt.debug_last_start()["ran_inline"] == value
    assert_bits(got, oracle.render(hs, params), f"random-spheres 40x24, start_inline {value}")


# ---- A: the walk in the reference's order keeps its own leaf bounds -----------------------------------------------------------------
def test_the_reference_order_walk(rt, oracle, gpu):
    hs = base_scene(rt, 40, 24)
    params = rt.render_params(seed=5)
    got = rt.DeviceScene(hs, walk=rt.RT_WALK_REFERENCE_ORDER).render(params)
    assert rt.debug_last_kernel()["ordered"] == 0
    assert_bits(got, oracle.render(hs, params), "random-spheres 40x24 in the reference's order")


# ---- the stack: deepest, shallowest, frame exits ---------------------------------------------------------------------------------------------
def _render_32x24(rt, oracle, hs, what, **opts):
    cam = rt.Camera.from_buffer_copy(bytes(hs.camera))
    params = rt.render_params(seed=8, sample_end=2)
    ds = rt.DeviceScene(hs, **opts)
    got = ds.render(params, camera=cam)
    assert_bits(got, oracle.render(hs, params, camera=cam), what)
    return ds.stats()


def test_the_deepest_and_the_shallowest_stack(rt, oracle, gpu):
    deepest = None
    for cls, (name, opts, k) in kc.CLASSES.items():
        if k["ordered"] and name in ("spheres300", "spheres1200", "spheres6000"):
            o = dict(opts, walk=getattr(rt, opts["walk"]))
            layout = rt.debug_wide_layout if o.get("wide") else rt.debug_ordered_layout
            depth = layout(kc.scene(rt, name), **o)["stack_entries"]
            if deepest is None or depth > deepest[0]:
                deepest = (depth, cls)
    depth, cls = deepest
    assert depth > 4, deepest
    name, opts, _ = kc.CLASSES[cls]
    st = _render_32x24(rt, oracle, kc.scene(rt, name), f"{cls}: stack of {depth}", **dict(opts, walk=getattr(rt, opts["walk"])))
    assert st["stack_entries"] >= 4, st
    cam = look(rt, 32, 24, (0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 2)
    one = custom_scenes.single_sphere_scene(_Aimed(cam))
    st = _render_32x24(rt, oracle, one, "one sphere")
    assert st["stack_entries"] <= 1, st


def test_frame_exits_are_popped_from_the_stack(rt, oracle, gpu):
    hs = kc.scene(rt, "cornell_smoke")
    params = rt.render_params(seed=8, sample_end=2)
    assert_bits(rt.DeviceScene(hs).render(params), oracle.render(hs, params), "cornell_smoke")
    cam = look(rt, 32, 24, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 2)
    nested = custom_scenes.nested_frames_scene(_Aimed(cam))
    st = _render_32x24(rt, oracle, nested, "instances inside instances")
    assert st["max_instance_depth"] >= 2, st


# ---- the choice among four children ---------------------------------------------------------------------------------------------------
LAMPS = [(4.0, 0.5, 0.5), (0.5, 4.0, 0.5), (0.5, 0.5, 4.0), (3.0, 3.0, 0.5)]


def four_lamps(rt, look_from, look_at):
    """four lamps of four colours around the view's axis on a black background.  Padded with spheres far behind the camera to 64
    primitives and more, so that the four-child kernel renders it."""
    cam = look(rt, 16, 16, look_from, look_at, 2)
    s = custom_scenes.CustomScene(_Aimed(cam), spp=2, depth=DEPTH, background=(0.0, 0.0, 0.0))
    items = [s.sphere(c, 0.9, s.light(*LAMPS[k])) for k, c in enumerate([(-1.5, 1.5, 0.0), (1.5, 1.5, 0.0), (-1.5, -1.5, 0.0), (1.5, -1.5, 0.0)])]
    grey = s.lambertian(0.5, 0.5, 0.5)
    for k in range(64):
        items.append(s.sphere((-8.0 + 0.25 * k, -6.0, 30.0 + (k % 5)), 0.1, grey))
    return s.finish(s.list(items))


def test_every_child_slot_is_chosen(rt, oracle, gpu):
    import torch
    hs = four_lamps(rt, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0))
    params = rt.render_params(seed=2)
    want = oracle.render(hs, params)
    px = want.reshape(-1, 3)
    for k, colour in enumerate(LAMPS):  # (2 samples of a pixel wholly inside a lamp's disc sum to twice its colour)
        assert (px == 2.0 * np.array(colour)).all(-1).any(), f"no pixel shows lamp {k} alone"
    ds = rt.DeviceScene(hs)
    d = torch.zeros(16 * 16 * 3, dtype=torch.float64, device="cuda")
    ds.render_device_counted(params, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rt.debug_last_kernel()["wide"] == 1 and rt.debug_last_kernel()["features"] == rt.RT_FEAT_SPHERES_SOLID
    assert rt.debug_visit_stats()["first"] > 0
    assert_bits(d.cpu().numpy(), want, "four lamps, counted render")
    assert_bits(ds.render(params), want, "four lamps")


def test_rays_along_an_axis_enter_every_child(rt, oracle, gpu):
    """the camera looks exactly down -z from a point on the z axis: the centre column's and row's rays have a zero direction component"""
    hs = four_lamps(rt, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0))
    cam = rt.Camera.from_buffer_copy(bytes(hs.camera))
    v = lambda a: np.array([a.x, a.y, a.z])
    # the middle of pixel (8, 8) put exactly on the axis: its ray is (0, 0, -z), degenerate on two axes
    shift = v(cam.pixel00_loc) + 8 * v(cam.pixel_delta_u) + 8 * v(cam.pixel_delta_v) - v(cam.center)
    cam.pixel00_loc = type(cam.pixel00_loc)(cam.pixel00_loc.x - shift[0], cam.pixel00_loc.y - shift[1], cam.pixel00_loc.z)
    params = rt.render_params(seed=2)
    want = oracle.render(hs, params, camera=cam)
    assert_bits(rt.DeviceScene(hs).render(params, camera=cam), want, "four lamps, rays along the axes")
    assert rt.debug_last_kernel()["wide"] == 1


# ---- the job modes: the flagship kernel's twins --------------------------------------------------------------------------------------
def test_a_pixel_list_and_three_views_of_random_spheres(rt, oracle, gpu):
    import torch
    w, h = 32, 24
    hs = base_scene(rt, w, h)
    ds = rt.DeviceScene(hs)
    want = oracle.render(hs, rt.render_params(seed=7)).reshape(w * h, 3)
    pixels, chosen = kc.stress_list(w * h)
    lst = torch.from_numpy(pixels.view(np.int32)).cuda()
    s = torch.full((w * h * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    ds.render_pixels_device(rt.render_params(seed=7, sample_end=4), lst.data_ptr(), pixels.size, s.data_ptr(), 0,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rt.debug_last_kernel() == dict(SPHERES_WIDE, features=rt.RT_FEAT_SPHERES_SOLID, jobs=rt.RT_JOBS_LIST)
    got = s.cpu().numpy().reshape(w * h, 3)
    mask = np.zeros(w * h, dtype=bool)
    mask[chosen] = True
    assert_bits(got[mask], want[mask], "list mode")
    assert (bits(got[~mask]) == SENTINEL).all()
    views = (rt.View * 3)()
    for k, look_from in enumerate([(13.0, 2.0, 3.0), (6.0, 3.0, 9.0), (-5.0, 1.5, 8.0)]):
        cam = rt.camera_look(hs, look_from, None)
        views[k].camera, views[k].seed = cam, 30 + k
    got = ds.render_views(rt.render_params(sample_end=4), views)
    assert rt.debug_last_kernel() == dict(SPHERES_WIDE, features=rt.RT_FEAT_SPHERES_SOLID, jobs=rt.RT_JOBS_VIEWS)
    for k in range(3):
        cam = rt.Camera.from_buffer_copy(bytes(views[k].camera))
        assert_bits(got[k].reshape(-1), oracle.render(hs, rt.render_params(seed=30 + k, sample_end=4), camera=cam), f"view {k}")
