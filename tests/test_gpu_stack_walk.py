"""The ordered walk's stack as the kernels hold it (rt_kernel.hip): the position is the ADDRESS of the lane's next free entry, "empty" is
a compare against the lane's level-0 entry, and a four-child record's entry carries, above the index, the children that are NOT to be
looked at any more (a record come to for the first time is its bare index).  The stock scenes rarely fill the stack; these do.

The row: 64 overlapping spheres along the z axis, one sphere per leaf, seen end-on from a camera on the axis.  A ray down the axis
passes through every sphere, so it enters several children of every record it comes to, and the first descent — nearest child first,
the others set aside — fills one entry per level before any primitive is tested.  That depth is worked out here on the CPU from the
scene compiler's records (debug_wide_records) for the ray through the frame's middle and must equal the scene's stack_entries: the
walk reaches the bound.  Rendered by the two four-child-record kernels a spheres scene reaches (records in the LDS: spheres_solid,
level 3; forced out of the LDS: the every-feature kernel, level 0) in the dense, pixel-list and views job modes.

One record only (four spheres): whatever is not entered leaves nothing on the stack, so the first pop finds it empty — at the lane's
base address — on the first visit.  The same four spheres as a two-child tree run visit_record with the same stack.

Every frame is 32x24 at 4 samples, depth 8, and is held to the CPU oracle bit for bit; rt_debug_last_kernel says which kernel ran."""
import numpy as np
import pytest

import custom_scenes
from adaptive_helpers import PAD, SENTINEL, assert_bits, bits

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 32, 24, 4, 8
OREF_KIND_SHIFT, OREF_INDEX_MASK, OK_INNER, OK_EMPTY = 29, (1 << 26) - 1, 0, 7  # rt_layout.h
ROW_OPTS = dict(leaf_max=1, flat_max=0, wide=1)
CELLS = {  # what rt_debug_last_kernel reports, but for the job mode
    "lds3": (dict(), dict(features=1, lds_level=3, ordered=1, wide=1, threads=1024)),
    "lds0": (dict(use_lds=0), dict(features=31, lds_level=0, ordered=1, wide=1, threads=256)),
}
JOBS = {"dense": 0, "list": 1, "views": 2}
_cache = {}


class _Aimed:
    def __init__(self, camera):
        self.camera = camera


def camera(rt, look_from, look_at):
    if "base" not in _cache:
        _cache["base"] = rt.HostScene(0, width=W, aspect=W / H, spp=SPP, depth=DEPTH)
        assert (_cache["base"].width, _cache["base"].height) == (W, H)
    cam = rt.camera_look(_cache["base"], look_from, look_at)
    cam.samples_per_pixel, cam.max_depth, cam.defocus_angle = SPP, DEPTH, 0.0
    return cam


def row_scene(rt):
    if "row" not in _cache:
        s = custom_scenes.CustomScene(_Aimed(camera(rt, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))), spp=SPP, depth=DEPTH, background=(0.7, 0.8, 1.0))
        mats = [s.dielectric(1.5), s.lambertian(0.8, 0.3, 0.3), s.metal(0.8, 0.8, 0.9, 0.0), s.dielectric(1.3), s.lambertian(0.3, 0.4, 0.8)]
        # (radii that differ a little, so that no two boxes are entered at exactly the same distance)
        _cache["row"] = s.finish(s.list([s.sphere((0.0, 0.0, -0.35 * k), 0.5 + 0.003 * (k % 7), mats[k % len(mats)]) for k in range(64)]))
    return _cache["row"]


def four_spheres_scene(rt):
    if "four" not in _cache:
        s = custom_scenes.CustomScene(_Aimed(camera(rt, (0.0, 1.0, 6.0), (0.0, 0.0, 0.0))), spp=SPP, depth=DEPTH, background=(0.7, 0.8, 1.0))
        mats = [s.lambertian(0.8, 0.3, 0.3), s.metal(0.8, 0.8, 0.9, 0.0), s.dielectric(1.5), s.lambertian(0.3, 0.8, 0.3)]
        _cache["four"] = s.finish(s.list([s.sphere((-2.4 + 1.6 * k, 0.2 * k, -0.5 * k), 0.7, mats[k]) for k in range(4)]))
    return _cache["four"]


def first_descent_depth(rec, root, o, d):
    """entries on the stack when the walk of ray (o, d) from record `root` first comes to a leaf: nearest entered child first, the
    record set aside wherever another child is entered too (interval (0.001, inf): nothing has been hit yet)"""
    depth, node = 0, root
    while True:
        enter = []
        for k in range(4):
            if (int(rec["refs"][node, k]) >> OREF_KIND_SHIFT) == OK_EMPTY:
                continue
            b = rec["boxes"][node, k].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (b[:, 0] - o) / d, (b[:, 1] - o) / d
            en, le = max(np.minimum(t0, t1).max(), 0.001), np.maximum(t0, t1).min()
            if en <= le:
                enter.append((en, k))
        assert enter, "the ray misses every child of a record on its way down"
        depth += 1 if len(enter) > 1 else 0
        ref = int(rec["refs"][node, min(enter)[1]])
        if (ref >> OREF_KIND_SHIFT) != OK_INNER:
            return depth
        node = ref & OREF_INDEX_MASK


def middle_ray(cam):
    v = lambda a: np.array([a.x, a.y, a.z])
    return v(cam.center), v(cam.pixel00_loc) + (W // 2) * v(cam.pixel_delta_u) + (H // 2) * v(cam.pixel_delta_v) - v(cam.center)


def oracle_frame(oracle, rt, hs, cam, seed):
    key = (id(hs), bytes(cam), seed)
    if key not in _cache:
        f = oracle.render(hs, rt.render_params(seed=seed), camera=rt.Camera.from_buffer_copy(bytes(cam)))
        f.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def render(rt, oracle, hs, mode, what, **opts):
    """one frame (two in views mode) in the given job mode against the oracle; returns the DeviceScene"""
    import torch
    ds = rt.DeviceScene(hs, **opts)
    n_pix = W * H
    if mode == "dense":
        assert_bits(ds.render(rt.render_params(seed=8)), oracle_frame(oracle, rt, hs, hs.camera, 8), what)
    elif mode == "list":
        g = np.random.default_rng(2)
        chosen = g.permutation(n_pix).astype(np.uint32)[: n_pix - 37]
        pixels = np.insert(chosen, g.integers(0, chosen.size, 5), PAD).astype(np.uint32)
        assert pixels.size % 64 != 0
        lst = torch.from_numpy(pixels.view(np.int32)).cuda()
        s = torch.full((n_pix * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
        q = torch.full((n_pix * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
        ds.render_pixels_device(rt.render_params(seed=8), lst.data_ptr(), len(pixels), s.data_ptr(), q.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got, want = s.cpu().numpy().reshape(n_pix, 3), np.asarray(oracle_frame(oracle, rt, hs, hs.camera, 8)).reshape(n_pix, 3)
        mask = np.zeros(n_pix, dtype=bool)
        mask[chosen] = True
        assert_bits(got[mask], want[mask], f"{what}: the listed pixels")
        assert (bits(got[~mask]) == SENTINEL).all(), f"{what}: an unlisted pixel was written"
    else:
        views = (rt.View * 2)()
        look_from = [(0.0, 0.0, 5.0), (0.4, 0.2, 5.0)] if hs is _cache.get("row") else [(0.0, 1.0, 6.0), (1.0, 0.5, 6.0)]
        for k in range(2):
            views[k].camera, views[k].seed = camera(rt, look_from[k], (0.0, 0.0, 0.0)), 8 + k
        d = torch.full((2 * n_pix * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
        ds.render_views_device(rt.render_params(sample_end=SPP), views, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d.cpu().numpy().reshape(2, -1)
        for k in range(2):
            assert_bits(got[k], np.asarray(oracle_frame(oracle, rt, hs, views[k].camera, 8 + k)).reshape(-1), f"{what}: view {k}")
    return ds


def check_kernel(rt, want, mode):
    got = rt.debug_last_kernel()
    assert {k: got[k] for k in list(want) + ["jobs"]} == dict(want, jobs=JOBS[mode]), got


def test_the_row_fills_the_stack_on_the_first_descent(rt):
    hs = row_scene(rt)
    rec, lay = rt.debug_wide_records(hs, **ROW_OPTS), rt.debug_wide_layout(hs, **ROW_OPTS)
    assert rec["wide"] and lay["violations"] == 0 and lay["records"] == len(rec["refs"]) >= 21, lay
    inner = rec["refs"][(rec["refs"] >> OREF_KIND_SHIFT) == OK_INNER] & OREF_INDEX_MASK
    (root,) = sorted(set(range(len(rec["refs"]))) - set(inner.tolist()))  # the one record that is nobody's child
    o, d = middle_ray(hs.camera)
    assert lay["stack_entries"] >= 3, lay
    assert first_descent_depth(rec, root, o, d) == lay["stack_entries"], lay


@pytest.mark.parametrize("mode", list(JOBS))
@pytest.mark.parametrize("cell", list(CELLS))
def test_a_full_stack_in_every_job_mode(rt, oracle, gpu, cell, mode):
    more, want = CELLS[cell]
    ds = render(rt, oracle, row_scene(rt), mode, f"the row, {cell}, {mode}", **ROW_OPTS, **more)
    check_kernel(rt, want, mode)
    assert ds.stats()["stack_entries"] == rt.debug_wide_layout(row_scene(rt), **ROW_OPTS)["stack_entries"]


@pytest.mark.parametrize("mode", list(JOBS))
@pytest.mark.parametrize("wide", [1, 0])
def test_a_tree_of_one_record_pops_an_empty_stack_on_the_first_visit(rt, oracle, gpu, wide, mode):
    hs = four_spheres_scene(rt)
    opts = dict(leaf_max=1, flat_max=0, wide=wide, start_shortcut=0)
    if wide:
        rec = rt.debug_wide_records(hs, **opts)
        assert rec["wide"] and len(rec["refs"]) == 1, rec["refs"]
    else:
        lay = rt.debug_ordered_layout(hs, **opts)
        assert lay["ordered"] and len(lay["nodes"]) == 3, lay["nodes"].shape
    render(rt, oracle, hs, mode, f"four spheres, wide {wide}, {mode}", **opts)
    check_kernel(rt, dict(features=1, lds_level=3, ordered=1, wide=wide, threads=1024), mode)
