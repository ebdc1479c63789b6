"""The four-child records (rt_layout.h ONode4) as the device sees them: rt_debug_wide_records returns, from the functions scene
creation itself runs, every record's slot boxes and references, the f64 bound of what each slot holds, the filter's B (box_extent)
and the two packed images that are uploaded.  CPU checks; the visit of such a record is checked in test_gpu_wide_visit.py."""
import numpy as np
import pytest

import custom_scenes
import scene_cases

KIND_EMPTY = 7
EMPTY_REF = KIND_EMPTY << 29


def hand_made(rt):
    cam = scene_cases.build(rt, "quads_64x64_8spp")
    return {"tie0": custom_scenes.tie_scene(cam, 0), "tie1": custom_scenes.tie_scene(cam, 1), "single_sphere": custom_scenes.single_sphere_scene(cam),
            "empty_frame": custom_scenes.empty_frame_scene(cam), "many_spheres_300": custom_scenes.many_spheres_scene(cam, 300),
            "media0": custom_scenes.media_scene(cam, 0), "media1": custom_scenes.media_scene(cam, 1), "media2": custom_scenes.media_scene(cam, 2),
            "nested_frames": custom_scenes.nested_frames_scene(cam), "random3": custom_scenes.random_scene(cam, 3),
            "random8": custom_scenes.random_scene(cam, 8), "many_media_20": custom_scenes.many_media_scene(cam, 20),
            "many_instances_40": custom_scenes.many_instances_scene(cam, 40)}


def unpack_global(img):
    """256-byte records -> (boxes (n, 4, 3, 2) from the "+" tables, the same from the "-" tables, refs (n, 4))."""
    n = img.shape[0]
    f = np.ascontiguousarray(img[:, :192]).view(np.float32).reshape(n, 3, 2, 2, 4)  # [record, axis, sign table, near / far, child]
    plus = np.stack([f[:, :, 0, 0, :], f[:, :, 0, 1, :]], axis=-1).transpose(0, 2, 1, 3)   # near = lo, far = hi
    minus = np.stack([f[:, :, 1, 1, :], f[:, :, 1, 0, :]], axis=-1).transpose(0, 2, 1, 3)  # near = hi, far = lo
    refs = np.ascontiguousarray(img[:, 192:208]).view(np.uint32).reshape(n, 4)
    return plus, minus, refs


def unpack_lds(img, n, table_bytes):
    """six plane tables of table_bytes and the reference table -> the same three arrays."""
    assert table_bytes == 32 * n and img.size == 208 * n
    t = np.ascontiguousarray(img[:6 * table_bytes]).view(np.float32).reshape(3, 2, n, 2, 4)  # [axis, sign table, record, near / far, child]
    plus = np.stack([t[:, 0, :, 0, :], t[:, 0, :, 1, :]], axis=-1).transpose(1, 2, 0, 3)
    minus = np.stack([t[:, 1, :, 1, :], t[:, 1, :, 0, :]], axis=-1).transpose(1, 2, 0, 3)
    refs = np.ascontiguousarray(img[6 * table_bytes:]).view(np.uint32).reshape(n, 4)
    return plus, minus, refs


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check(rec, what, min_records=1):
    assert rec["wide"], what
    boxes, refs, bounds = rec["boxes"], rec["refs"], rec["bounds"]
    n = len(boxes)
    assert n >= min_records and rec["table_bytes"] == 32 * n, what
    empty = (refs >> 29) == KIND_EMPTY
    # every slot that holds something: its f32 box contains the f64 bound of what it holds (and that bound is a box)
    held = bounds[~empty]
    assert np.isfinite(held).all() and (held[..., 0] <= held[..., 1]).all(), what
    b64 = boxes[~empty].astype(np.float64)
    assert np.isfinite(b64).all(), what
    bad = (b64[..., 0] > held[..., 0]) | (b64[..., 1] < held[..., 1])
    assert not bad.any(), (what, np.argwhere(bad)[:4], b64[bad.any(axis=-1)][:2], held[bad.any(axis=-1)][:2])
    # every empty slot: exactly lo = +inf, hi = -inf on all axes, the empty reference, and nothing held
    assert (refs[empty] == EMPTY_REF).all(), what
    assert np.isposinf(boxes[empty][..., 0]).all() and np.isneginf(boxes[empty][..., 1]).all(), what
    assert np.isposinf(bounds[empty][..., 0]).all() and np.isneginf(bounds[empty][..., 1]).all(), what
    assert (~empty).any(axis=1).sum() >= n - 1, what  # (only a scene with nothing to hit has a record of four empty slots)
    # the filter's precondition: |plane| <= B for every plane it is ever given
    B = np.float64(rec["box_extent"])
    assert np.isfinite(B), what
    if (~empty).any():
        assert np.abs(b64).max() <= B, (what, np.abs(b64).max(), B)
    steps = rec["step_boxes"].astype(np.float64)
    assert len(steps) >= 1 and np.isfinite(steps).all() and np.abs(steps).max() <= B, (what, steps, B)
    # the packed images round-trip: both sign tables of every axis and the reference table, in both forms
    for form, (plus, minus, r) in (("global", unpack_global(rec["global_image"])), ("lds", unpack_lds(rec["lds_image"], n, rec["table_bytes"]))):
        assert same_bits(plus, boxes), (what, form, "+ tables")
        assert same_bits(minus, boxes), (what, form, "- tables")
        assert np.array_equal(r, refs), (what, form, "references")
    return int(empty.sum()), n


@pytest.mark.parametrize("name", list(scene_cases.CASES))
def test_wide_records_of_every_case(rt, name):
    hs = scene_cases.build(rt, name)
    prims = rt.debug_ordered_layout(hs)
    rec = rt.debug_wide_records(hs, wide=1, walk=rt.RT_WALK_OWN_TREES)
    assert rec["wide"] == prims["ordered"], name
    check(rec, name)
    # the default options give four-child records exactly to the scenes of 64 primitives or more that get the ordered walk
    default = rt.debug_wide_records(hs)
    n_prims = len(prims["spheres"]) + len(prims["quads"])
    assert default["wide"] == (n_prims >= 64), (name, n_prims)
    assert rt.debug_wide_records(hs, wide=0)["wide"] is False and len(rt.debug_wide_records(hs, wide=0)["boxes"]) == 0
    if default["wide"]:
        assert same_bits(default["boxes"], rec["boxes"]) and np.array_equal(default["global_image"], rec["global_image"])
        assert rt.debug_wide_layout(hs)["records"] == len(rec["boxes"])


def test_wide_records_of_the_hand_made_scenes(rt):
    empties = records = 0
    for name, scene in hand_made(rt).items():
        rec = rt.debug_wide_records(scene, wide=1, walk=rt.RT_WALK_OWN_TREES)
        if not rt.debug_ordered_layout(scene)["ordered"]:
            assert not rec["wide"], name
            continue
        e, n = check(rec, name)
        empties += e; records += n
        for opts in ({"flat_max": 0}, {"leaf_max": 4}):
            check(rt.debug_wide_records(scene, wide=1, walk=rt.RT_WALK_OWN_TREES, **opts), (name, opts))
    assert records >= 100 and empties >= 20, (records, empties)  # (the checks of empty slots saw some)


def test_the_checks_can_fail(rt):
    """The round trip and the containment are not vacuous: a record with one plane moved, or one table entry swapped, is caught."""
    rec = rt.debug_wide_records(scene_cases.build(rt, "c2_random_balls_96x64_8spp_d50"), wide=1)
    assert len(rec["boxes"]) >= 100
    moved = dict(rec); moved["boxes"] = rec["boxes"].copy()
    slot = np.argwhere((rec["refs"] >> 29) != KIND_EMPTY)[7]
    moved["boxes"][slot[0], slot[1], 1, 1] = np.nextafter(np.float32(rec["bounds"][slot[0], slot[1], 1, 1]), np.float32(-np.inf)) - np.float32(1e-3)
    with pytest.raises(AssertionError):
        check(moved, "moved plane")
    swapped = dict(rec); swapped["lds_image"] = rec["lds_image"].copy()
    off = 3 * rec["table_bytes"] + 32 * 5  # the Y- table, record 5: children 0 and 1 of the near planes
    swapped["lds_image"][off:off + 8] = np.concatenate([rec["lds_image"][off + 4:off + 8], rec["lds_image"][off:off + 4]])
    if not np.array_equal(swapped["lds_image"], rec["lds_image"]):
        with pytest.raises(AssertionError):
            check(swapped, "swapped table entry")
    small = dict(rec); small["box_extent"] = float(np.nextafter(np.float32(rec["box_extent"]), np.float32(0)))
    with pytest.raises(AssertionError):
        check(small, "extent one ulp short")


def test_the_visit_generator_carries_the_floors_of_the_gpu_test(rt):
    """tests/test_gpu_wide_visit.py asserts floors on how many cases exercised each property; here its generator and its numpy
    reference run alone (no GPU) and must give at least twice each floor — and the share of rejections its filter test relies on."""
    import test_gpu_wide_visit as W
    n = W.N_BASE
    c = W.gen_cases(n, 2024)
    exists, todo = ~c["empty"], W.todo_bits(c["todo"])
    floors = W.expected_floors(n)
    for tmin, tmax in W.INTERVALS[:3]:
        want = W.ref_enters(c["rays"], c["boxes"], tmin, tmax) & exists & todo
        assert want[:, 2:].sum() >= 2 * floors["second_half"], (tmin, tmax, want[:, 2:].sum())
    assert (c["empty"] & todo).sum() >= 2 * floors["empty_tested"]
    degenerate = W.surely_degenerate(c["rays"])
    assert degenerate.sum() >= 2 * floors["degenerate"] and (degenerate[:, None] & c["empty"] & todo).sum() >= 2 * 0.01 * n
    # identical boxes in two slots that the reference enters and todo holds: their keys tie
    want = W.ref_enters(c["rays"], c["boxes"], 0.001, np.inf) & exists & todo
    same = (c["boxes"][:, :, None] == c["boxes"][:, None, :]).all(axis=(3, 4))
    tie = np.zeros(n, dtype=bool)
    for i in range(4):
        for j in range(i + 1, 4):
            tie |= same[:, i, j] & want[:, i] & want[:, j]
    assert tie.sum() >= 2 * 0.01 * n, tie.sum()
    # every mask value and every number of empty slots occurs
    assert set(np.unique(c["todo"])) == set(range(16)) and set(np.unique(c["empty"].sum(axis=1))) == {0, 1, 2, 3}
    # the filter test's rays: the reference rejects well over 0.2 of the slots that exist
    f = W.gen_cases(200_000, 99, aimed=False)
    rejected = ~W.ref_enters(f["rays"], f["boxes"], 0.001, np.inf) & ~f["empty"]
    assert rejected.sum() > 0.4 * (~f["empty"]).sum(), rejected.sum()
