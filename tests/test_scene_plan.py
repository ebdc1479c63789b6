"""The scene plan (csrc/rt_scene_plan.hpp, seen through rt_debug_scene_plan; no GPU): what rt_scene_create_ex decides and uploads.

Pins: every digest, size and scalar of tests/golden/scene_plan_pins.json, recorded from scene creation as it was before it was
split into plan and upload (scene_plan_cases.py says how).  Properties: the layout rules, restated here from the struct sizes."""
import struct

import numpy as np
import pytest

import custom_scenes
import kernel_classes as kc
import scene_plan_cases as spc

LDS_BUDGET = 160 * 1024                      # rt_kernels.h LDS_BUDGET_BYTES
SPHERE, QUAD, QFILT, OSEQ, INSTANCE, MEDIUM, MATERIAL = 64, 144, 112, 112, 128, 16, 64   # rt_layout.h / rt_kernels.h struct sizes
WIDE_MAX_LDS_RECORDS = 4094                  # rt_layout.h
FEATS = (1, 6, 14, 19)                       # rt_kernels.h FEAT_*: the specialised kernels of LDS level 3
_plans = {}


def plan_of(rt, name, option_set):
    if (name, option_set) not in _plans:
        _plans[name, option_set] = rt.debug_scene_plan(spc.scene(rt, name), **spc.options(rt, option_set))
    return _plans[name, option_set]


def align16(x):
    return (x + 15) & ~15


@pytest.fixture(scope="module")
def pins():
    return spc.pins()


def test_the_pins_cover_every_case(pins):
    assert sorted(pins) == sorted(spc.key(*c) for c in spc.cases())
    assert len(spc.STOCK) == 9 and len(spc.OPTION_SETS) == 3


@pytest.mark.parametrize("name,option_set", spc.cases(), ids=lambda v: v)
def test_plan_reproduces_the_pinned_scene_creation(rt, pins, name, option_set):
    want, got = pins[spc.key(name, option_set)], plan_of(rt, name, option_set)
    scalars = {k: got[k] for k in rt.PLAN_SCALARS if k not in ("box_extent", "lds_prefix_bytes", "aux_off")}
    scalars["box_extent_bits"] = struct.unpack("<I", struct.pack("<f", got["box_extent"]))[0]
    scalars.update({f"lds_prefix_bytes_{k}": v for k, v in enumerate(got["lds_prefix_bytes"])})
    scalars.update({f"aux_off_{k}": v for k, v in enumerate(got["aux_off"])})
    assert scalars == want["scalars"]
    assert got["stats"] == want["stats"]
    assert {k: [got["sizes"][k], got["digests"][k]] for k in got["sizes"]} == want["arrays"]
    for k in rt.PLAN_IMAGES:  # the bytes handed out are the bytes digested
        assert got[k].size == got["sizes"][k]
        h = 0xcbf29ce484222325
        for b in got[k][:4096].tobytes():
            h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
        if got[k].size <= 4096:
            assert f"{h:016x}" == got["digests"][k]


def kernel_features(features, lds):
    if lds == 3:
        for f in FEATS:
            if features & ~f == 0:
                return f
    return 31


def threads(kf, lds, ordered):
    if lds == 0:
        return 256
    return 768 if (kf == 19 and not ordered) else 1024


@pytest.mark.parametrize("name,option_set", spc.cases(), ids=lambda v: v)
def test_regions_of_the_dynamic_lds(rt, name, option_set):
    """image prefix | stacks | sequence | AUX | world rays | profile rows: 16-byte aligned, in this order, each present part as large
    as its contents, within 160 KiB"""
    p = plan_of(rt, name, option_set)
    level = p["lds_level"]
    assert sorted(p["levels"]) == sorted({0, level})
    prefix = p["lds_prefix_bytes"]
    assert prefix[0] == 0 and all(prefix[k] <= prefix[k + 1] for k in range(level)) and all(v == 0 for v in prefix[level + 1:])
    if level:
        assert prefix[level] == p["sizes"]["lds_image"]
    assert p["sizes"]["aux_image"] == p["aux_bytes"]
    assert p["aux_off"] == sorted(p["aux_off"]) and all(o % 16 == 0 for o in p["aux_off"] + [p["aux_bytes"]])
    for off in ("lds_off_node_b", "lds_off_spheres", "lds_off_quads", "lds_off_qfilt"):
        assert p[off] % 16 == 0
    for lds, v in p["levels"].items():
        kf = kernel_features(p["features"], lds)
        th = threads(kf, lds, p["ordered"])
        assert (v["features"], v["threads"]) == (kf, th)
        stack = p["o_stack"] * th * (2 if lds else 4) if p["ordered"] else 0
        prof = th // 64 * 12 * 3 * 8
        assert v["stack_off"] == prefix[lds]
        assert v["seq_off"] == align16(prefix[lds] + stack)
        assert v["aux_off"] == align16(v["seq_off"] + (p["n_oseq"] * OSEQ if p["ordered"] else 0))
        aux = bool(p["ordered"] and p["aux_bytes"] and v["aux_off"] + p["aux_bytes"] + prof <= LDS_BUDGET)
        assert v["aux_in_lds"] == aux
        assert v["world_off"] == align16(v["aux_off"] + (p["aux_bytes"] if aux else 0))
        world = bool(p["has_instances"] and v["world_off"] + 48 * th + prof <= LDS_BUDGET)
        assert v["world_in_lds"] == world
        assert v["prof_off"] == v["world_off"] + (48 * th if world else 0)
        assert (v["dynamic_lds_bytes"], v["dynamic_lds_bytes_counted"]) == (v["prof_off"], v["prof_off"] + prof)
        for off in ("stack_off", "seq_off", "aux_off", "world_off", "prof_off"):
            assert v[off] % 16 == 0
        assert v["dynamic_lds_bytes_counted"] <= LDS_BUDGET
    assert p["stats"]["lds_bytes"] == (p["levels"][level]["dynamic_lds_bytes"] if level else 0)


def records_of(p):
    return p["stats"]["n_nodes"] if p["ordered"] else p["sizes"]["nodes"] // 32


def table_bytes(p):
    n = records_of(p)
    return n * 208 if p["wide"] else align16(n * 104) if p["ordered"] else n * 32


@pytest.mark.parametrize("name,option_set", spc.cases(), ids=lambda v: v)
def test_lds_level_is_the_largest_that_fits_the_documented_budget(rt, name, option_set):
    """budget = 160 KiB - 4 KiB - the sequence; level 3: the whole image (with the quad filter records where a leaf holds several quads
    and they fit too) plus the stacks of that level's kernel; else level 1: the node tables plus stacks; else 0.  Own trees whose record
    index does not fit a 2-byte stack entry: 0."""
    p = plan_of(rt, name, option_set)
    st = p["stats"]
    off_sph = table_bytes(p)
    assert p["lds_off_node_b"] == records_of(p) * (32 if p["wide"] else 16)
    off_quads = off_sph + st["n_spheres"] * SPHERE
    off_qfilt = align16(off_quads + st["n_quads"] * QUAD)
    budget = LDS_BUDGET - 4096 - p["n_oseq"] * OSEQ
    stack = {lds: p["o_stack"] * threads(kernel_features(p["features"], lds), lds, True) * 2 if p["ordered"] else 0 for lds in (1, 3)}
    too_many = p["ordered"] and records_of(p) >= (WIDE_MAX_LDS_RECORDS if p["wide"] else 0x3fff)
    filt = p["lds_off_qfilt"] != 0
    if filt:
        assert p["lds_level"] == 3 and p["lds_off_qfilt"] == off_qfilt and p["ordered"]
    total = off_qfilt + (st["n_quads"] * QFILT if filt else 0)
    want = 0 if too_many else 3 if total + stack[3] <= budget else 1 if off_sph + stack[1] <= budget else 0
    assert p["lds_level"] == want
    if want:
        assert (p["lds_off_spheres"], p["lds_off_quads"]) == (off_sph, off_quads)
        assert p["lds_prefix_bytes"][1:want + 1] == [off_sph, align16(off_quads), total][:want]


@pytest.mark.parametrize("name", list(spc.SCENES))
def test_node_tables_are_the_wide_hooks(rt, name):
    """four-child records: the global image and the head of the LDS image are what rt_debug_wide_records packs"""
    p = plan_of(rt, name, "own-wide1")
    w = rt.debug_wide_records(spc.scene(rt, name), **spc.options(rt, "own-wide1"))
    assert bool(p["wide"]) == w["wide"]
    if not w["wide"]:
        return
    assert np.array_equal(p["oimage"], w["global_image"].reshape(-1))
    assert p["lds_off_node_b"] == w["table_bytes"]
    if p["lds_level"]:
        assert np.array_equal(p["lds_image"][:w["lds_image"].size], w["lds_image"])


@pytest.mark.parametrize("name", list(spc.SCENES))
def test_node_tables_are_the_ordered_layouts_records(rt, name):
    """two-child records: rebuilt here from rt_debug_ordered_layout_ex's records — per axis the planes (lo0, lo1, hi0, hi1) and
    (hi0, hi1, lo0, lo1), then the two references; side by side in a 128-byte line of the global image"""
    p = plan_of(rt, name, "own-wide0")
    if not p["ordered"]:
        return
    nodes = rt.debug_ordered_layout(spc.scene(rt, name), **{k: v for k, v in spc.options(rt, "own-wide0").items() if k in ("leaf_max", "flat_max")})["nodes"]
    n = len(nodes)
    assert n == p["stats"]["n_nodes"]
    b0, b1, c = nodes[:, 0:6], nodes[:, 6:12], nodes[:, 12:14]
    planes = []
    for ax in range(3):
        lo0, hi0, lo1, hi1 = b0[:, 2 * ax], b0[:, 2 * ax + 1], b1[:, 2 * ax], b1[:, 2 * ax + 1]
        planes += [np.stack([lo0, lo1, hi0, hi1], 1), np.stack([hi0, hi1, lo0, lo1], 1)]
    tables = np.concatenate([t.reshape(-1) for t in planes] + [c.reshape(-1)]).astype(np.uint32)
    lines = np.zeros((n, 32), dtype=np.uint32)
    for q in range(6):
        lines[:, 4 * q:4 * q + 4] = planes[q]
    lines[:, 24:26] = c
    assert np.array_equal(p["oimage"].view(np.uint32), lines.reshape(-1))
    if p["lds_level"]:
        assert np.array_equal(p["lds_image"][:tables.size * 4].view(np.uint32), tables)


# ---- start shortcut, on small hand-made scenes ----
def _aimed(rt):
    return kc._Aimed(kc.aimed_camera(rt, kc.LOOK_FROM[0]))


def test_ground_sphere_starts_in_the_sphere_stage(rt):
    """(flat_max = 0: a frame of so few primitives would otherwise keep all seven in one flat leaf — and start there, in a seven-sphere range)"""
    hs = custom_scenes.many_spheres_scene(_aimed(rt), 6)
    flat = rt.debug_scene_plan(hs, walk=rt.RT_WALK_OWN_TREES, wide=0)
    assert (flat["o_start_stage"], flat["o_start_prim"], flat["o_start_end"]) == (1, 0, 7)
    for wide in (0, 1):
        p = rt.debug_scene_plan(hs, walk=rt.RT_WALK_OWN_TREES, wide=wide, flat_max=0)
        assert p["ordered"] == 1 and p["wide"] == wide
        assert p["o_start_stage"] == 1 and p["o_start_end"] == p["o_start_prim"] + 1
    # four-child records: what is set aside is the mask of the root's other children; the one other child itself where it is the
    # only one and an inner record.  (The tree builder fills a root up to four children, so with today's trees a lone inner sibling
    # does not occur — every size below takes the mask branch; the other is held to the rule all the same.)
    for n in (6, 9, 40):
        hs = custom_scenes.many_spheres_scene(_aimed(rt), n)
        p = rt.debug_scene_plan(hs, walk=rt.RT_WALK_OWN_TREES, wide=1, flat_max=0)
        root = rt.debug_wide_records(hs, walk=rt.RT_WALK_OWN_TREES, wide=1, flat_max=0)["refs"][p["o_root"]]
        others = {k: int(r) for k, r in enumerate(root) if k != p["o_start_slot"] and r >> 29 != 7}
        assert p["o_start_stage"] == 1 and p["o_start_end"] == p["o_start_prim"] + 1
        assert int(root[p["o_start_slot"]]) == (1 << 29) | p["o_start_prim"]
        assert p["o_start_rest"] == sum(1 << k for k in others)
        only = list(others.values())[0] if len(others) == 1 else None
        assert p["o_start_direct"] == (only & ((1 << 26) - 1) if only is not None and only >> 29 == 0 else 0xffffffff)


def test_a_box_in_a_translate_frame_starts_in_its_leaf(rt):
    s = custom_scenes.CustomScene(_aimed(rt))
    box = s.translate(s.list(custom_scenes._cube(s, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), s.lambertian(0.5, 0.5, 0.5))), (1.0, 0.0, 0.0))
    hs = s.finish(s.list([box, s.sphere((-2, 0, 0), 0.5, s.metal(0.8, 0.8, 0.8, 0.0)), s.sphere((-2, 2, 0), 0.5, s.dielectric(1.5))]))
    for wide in (0, 1):
        p = rt.debug_scene_plan(hs, walk=rt.RT_WALK_OWN_TREES, wide=wide)
        assert p["stats"]["n_instances"] == 1 and p["insts"].size == INSTANCE
        start_ref = int(p["insts"][56:60].view(np.uint32)[0])
        assert start_ref >> 29 == 2 and (start_ref >> 26) & 7 == 5 and start_ref & ((1 << 26) - 1) == 0  # six quads from quad 0
        box32 = p["insts"][64:88].view(np.float32)
        assert np.all(box32[0::2] <= np.float32(-0.5)) and np.all(box32[1::2] >= np.float32(0.5)) and np.all(np.abs(box32) < 0.5001)
        # the instance record in the AUX image is the one uploaded
        assert np.array_equal(p["aux_image"][p["aux_off"][2]:p["aux_off"][2] + INSTANCE], p["insts"])


def test_a_medium_takes_the_world_shortcut_away(rt):
    p = rt.debug_scene_plan(spc.scene(rt, "moving"), walk=rt.RT_WALK_OWN_TREES)
    assert p["ordered"] == 1 and p["stats"]["n_media"] > 0 and p["o_start_stage"] == 0
    q = rt.debug_scene_plan(custom_scenes.moving_scene(_aimed(rt), frames=False), walk=rt.RT_WALK_OWN_TREES)
    assert q["o_start_stage"] == 0


def test_one_primitive_is_not_ordered_under_the_default_walk(rt):
    hs = spc.scene(rt, "single_sphere")
    assert rt.debug_scene_plan(hs)["ordered"] == 0
    assert rt.debug_scene_plan(hs, walk=rt.RT_WALK_OWN_TREES)["ordered"] == 1


def _single_sphere_leaves(rt, n):
    s = custom_scenes.CustomScene(_aimed(rt))
    m = s.lambertian(0.5, 0.5, 0.5)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    return s.finish(s.list([s.sphere((k % side, k // side % side, k // (side * side)), 0.3, m) for k in range(n)]))


def test_wide_records_that_no_2_byte_entry_can_name_keep_the_scene_out_of_the_lds(rt):
    """single-sphere leaves (leaf_max = 1): a scene just large enough for WIDE_MAX_LDS_RECORDS records plans level 0; one sphere fewer
    stays below the limit and plans level 0 as well, for the reason worked out at the end"""
    opts = dict(walk=rt.RT_WALK_OWN_TREES, wide=1, leaf_max=1, flat_max=0)
    records = lambda n: rt.debug_scene_plan(_single_sphere_leaves(rt, n), **opts)["stats"]["n_nodes"]
    lo, hi = 3 * WIDE_MAX_LDS_RECORDS // 2, 4 * WIDE_MAX_LDS_RECORDS   # records(n) lies between n / 3 and n for n leaves
    assert records(lo) < WIDE_MAX_LDS_RECORDS <= records(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if records(mid) >= WIDE_MAX_LDS_RECORDS else (mid, hi)
    at, below = (rt.debug_scene_plan(_single_sphere_leaves(rt, n), **opts) for n in (hi, lo))
    assert below["stats"]["n_nodes"] < WIDE_MAX_LDS_RECORDS <= at["stats"]["n_nodes"]
    assert at["lds_level"] == 0
    # which reason applies one record short: do the node tables and the level-1 stacks fit the budget?
    budget = LDS_BUDGET - 4096 - below["n_oseq"] * OSEQ
    fits = below["stats"]["n_nodes"] * 208 + below["o_stack"] * 1024 * 2 <= budget
    # It is the size: 4093 records of 208 bytes are 851 344 bytes, five times the LDS.  (So the record limit never decides by itself.)
    assert not fits and below["lds_level"] == 0
