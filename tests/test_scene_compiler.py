"""The scene compiler inside librt_amd (object graph -> threaded records, box refit, f32 rounding), checked on the CPU
through rt_debug_compiled_nodes: the walk relies on these invariants to be allowed to skip a subtree."""
import numpy as np
import pytest

NK_INNER, NK_SPHERES, NK_QUADS, NK_INST_ENTER, NK_INST_EXIT, NK_MEDIUM_ENTER, NK_MEDIUM_EXIT, NK_MEDIUM_SPHERE = range(8)


def nodes_of(rt, scene, refit, **kw):
    hs = rt.HostScene(scene, spp=1, earth_image="synthetic:16x8", **kw)
    return hs, list(rt.debug_compiled_nodes(hs, refit))


@pytest.mark.parametrize("scene", range(9))
@pytest.mark.parametrize("bvh", ["reference", "sah"])
def test_threaded_links_and_containment(rt, scene, bvh):
    hs, nodes = nodes_of(rt, scene, True, bvh=bvh)
    n = len(nodes)
    assert n > 0
    for i, nd in enumerate(nodes):
        assert i < nd.skip <= n, (i, nd.skip)                     # links only go forward: the walk terminates
        # the f32 box the kernel tests contains the f64 box (outward rounding)
        for k in range(3):
            assert float(nd.lo32[k]) <= nd.lo[k] and nd.hi[k] <= float(nd.hi32[k])
        if nd.kind in (NK_SPHERES, NK_QUADS, NK_MEDIUM_SPHERE) and not nd.no_bbox:
            for k in range(3):                                     # a leaf's box contains its primitives
                assert nd.lo[k] <= nd.prim_lo[k] and nd.prim_hi[k] <= nd.hi[k], (i, k)

    # the box of an inner record contains the boxes of its direct children (same frame); a flat child (a quad) is
    # padded by 5e-5 on its thin axis (src/aabb.rs:35-53) and may stick out of a parent by that much: the parent
    # bounds the geometry, not the padding
    def check(i, end):
        k = i
        while k < end:
            nd = nodes[k]
            if nd.kind == NK_INNER:
                lo = np.array(nd.lo); hi = np.array(nd.hi)
                j = k + 1
                while j < nd.skip:
                    c = nodes[j]
                    if not c.no_bbox and not nd.no_bbox:
                        assert (lo <= np.array(c.lo) + 6e-5).all() and (np.array(c.hi) <= hi + 6e-5).all(), (k, j)
                    j = c.skip
                check(k + 1, nd.skip)
            elif nd.kind in (NK_INST_ENTER, NK_MEDIUM_ENTER):
                assert nodes[nd.skip - 1].kind in (NK_INST_EXIT, NK_MEDIUM_EXIT)   # brackets are balanced
                check(k + 1, nd.skip - 1)
            k = nd.skip
    check(0, n)
    d = hs.desc
    assert sum(nd.b for nd in nodes if nd.kind == NK_QUADS) >= d.n_quads
    assert sum(1 for nd in nodes if nd.kind in (NK_MEDIUM_ENTER, NK_MEDIUM_SPHERE)) == d.n_media


def test_refit_only_shrinks_boxes_and_fixes_the_origin_spanning_cubes(rt):
    hs, tight = nodes_of(rt, 8, True)
    _, loose = nodes_of(rt, 8, False)
    assert len(tight) == len(loose)
    spans_origin = lambda nd: all(nd.lo[k] <= 0.0 <= nd.hi[k] for k in range(3))
    shrunk = 0
    for a, b in zip(tight, loose):
        assert (a.kind, a.skip, a.a, a.b, a.no_bbox) == (b.kind, b.skip, b.a, b.b, b.no_bbox)
        if a.no_bbox:
            continue
        for k in range(3):
            assert b.lo[k] <= a.lo[k] and a.hi[k] <= b.hi[k]
        shrunk += a.hi[0] - a.lo[0] < b.hi[0] - b.lo[0]
    cubes_loose = [b for b in loose if b.kind == NK_QUADS and b.b == 6]
    cubes_tight = [a for a in tight if a.kind == NK_QUADS and a.b == 6]
    assert len(cubes_loose) == 400
    # the reference's cube lists all start from the all-zero default box (src/hittable.rs:50-57) ...
    assert all(spans_origin(b) for b in cubes_loose)
    # ... the refitted ones are the cubes themselves: 100 wide, and only the four around the origin touch it
    assert sum(spans_origin(a) for a in cubes_tight) <= 4
    assert all(abs((a.hi[0] - a.lo[0]) - 100.0) < 1e-6 for a in cubes_tight)
    assert shrunk > 400


def _motion_boxes(desc):
    """per sphere of the description: the box of the sphere at times 0, 0.5 and 1 — from the description alone"""
    out = []
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        c, vec, r = np.array(s.center.tuple()), np.array(s.center_vec.tuple()), abs(s.radius)
        at = [c + vec * t for t in ((0.0, 0.5, 1.0) if s.is_moving else (0.0,))]
        out.append((np.min([p - r for p in at], axis=0), np.max([p + r for p in at], axis=0)))
    return out


def _described(desc, centre, radius, vec, moving):
    """the description's spheres with exactly this geometry (coincident copies: more than one)"""
    return [i for i in range(desc.n_spheres) if desc.spheres[i].center.tuple() == tuple(centre) and desc.spheres[i].radius == radius and
            bool(desc.spheres[i].is_moving) == bool(moving) and (not moving or desc.spheres[i].center_vec.tuple() == tuple(vec))]


@pytest.mark.parametrize("n, frames", [(40, True), (3, False)])
def test_every_box_above_a_moving_sphere_holds_the_whole_motion(rt, n, frames):
    """custom_scenes.moving_scene: spheres that move along both directions of every axis and along the eight diagonals, by 1e-3 to 3
    radii, in the world, inside a frame and as media boundaries.  The box of a moving sphere is worked out HERE, from the description
    (times 0, 0.5 and 1); every record that holds the sphere, and every record above it, must contain it — in the threaded records, in
    the library's own trees of two children (leaf_max 1, 2, 4, 8) and of four (1, 3, 8).  (A flat list has no boxes of the
    reference's to intersect with: the threaded records of this scene carry the primitives' bound, not a box.)"""
    import custom_scenes
    import kernel_classes
    import test_ordered_layout as tol
    scene = custom_scenes.moving_scene(kernel_classes._Aimed(kernel_classes.aimed_camera(rt, kernel_classes.LOOK_FROM[0])), n=n, frames=frames)
    d = scene.desc
    boxes = _motion_boxes(d)
    n_moving = sum(d.spheres[i].is_moving for i in range(d.n_spheres))
    assert n_moving >= (n * 8) // 9 + 5 + (2 if frames else 0)
    moved = {tuple(np.sign(np.round(np.array(d.spheres[i].center_vec.tuple()), 9)).astype(int)) for i in range(d.n_spheres) if d.spheres[i].is_moving}
    assert n < 14 or len(moved) >= 14, "both directions of every axis and the eight diagonals"

    # the threaded records: the spheres are emitted in scan order, which is the order moving_scene makes them in
    nodes = list(rt.debug_compiled_nodes(scene, True))
    leaves = [nd for nd in nodes if nd.kind in (NK_SPHERES, NK_MEDIUM_SPHERE)]
    assert sum(nd.b if nd.kind == NK_SPHERES else 1 for nd in leaves) == d.n_spheres
    for nd in sorted(leaves, key=lambda nd: nd.a if nd.kind == NK_SPHERES else -1):
        if nd.kind != NK_SPHERES:
            continue
        lo = np.min([boxes[i][0] for i in range(nd.a, nd.a + nd.b)], axis=0); hi = np.max([boxes[i][1] for i in range(nd.a, nd.a + nd.b)], axis=0)
        assert (np.array(nd.prim_lo) <= lo).all() and (np.array(nd.prim_hi) >= hi).all(), (nd.a, nd.b)
        assert np.allclose(nd.prim_lo, lo, rtol=0, atol=1e-12) and np.allclose(nd.prim_hi, hi, rtol=0, atol=1e-12), (nd.a, nd.b)
        if not nd.no_bbox:
            assert (np.array(nd.lo) <= lo).all() and (np.array(nd.hi) >= hi).all(), (nd.a, nd.b)

    def check_tree(lay, slots_of, what):
        """slots_of(record) -> [(reference, f32 box (3, 2))]; returns the number of moving spheres met"""
        to_desc = [_described(d, row[0:3], row[3], row[4:7], row[8]) for row in lay["spheres"]]
        assert all(to_desc), (what, "a sphere of the layout is none of the description's: the motion was lost or changed")
        seen = [0]

        def under(record):
            lo_all, hi_all = np.full(3, np.inf), np.full(3, -np.inf)
            for ref, box in slots_of(record):
                kind, count, index = ref >> 29, ((ref >> 26) & 7) + 1, ref & ((1 << 26) - 1)
                if kind == tol.KIND_EMPTY:
                    continue
                if kind == tol.KIND_INNER:
                    lo, hi = under(index)
                elif kind == tol.KIND_INSTANCE:
                    inst = lay["instances"][index]
                    lo, hi = tol.to_parent(inst, *under(int(inst[7])))
                elif kind == tol.KIND_SPHERES:
                    held = [boxes[to_desc[index + i][0]] for i in range(count)]
                    lo, hi = np.min([b[0] for b in held], axis=0), np.max([b[1] for b in held], axis=0)
                    seen[0] += sum(bool(lay["spheres"][index + i, 8]) for i in range(count))
                else:
                    held = [tol.prim_bound(lay, kind, index + i) for i in range(count)]
                    lo, hi = np.min([b[0] for b in held], axis=0), np.max([b[1] for b in held], axis=0)
                assert (box[:, 0] <= lo).all() and (box[:, 1] >= hi).all(), (what, record, box, lo, hi)
                lo_all, hi_all = np.minimum(lo_all, lo), np.maximum(hi_all, hi)
            return lo_all, hi_all

        for step in lay["steps"]:
            kind, a, b = int(step[0]), int(step[1]), int(step[2])
            box = tol.f32_box(step[4:10])
            if kind == 1:  # a medium whose boundary is one sphere: the step's box is the sphere's
                index = int(lay["media"][a])
                lo, hi = boxes[to_desc[index][0]]
                seen[0] += bool(lay["spheres"][index, 8])
            else:
                lo, hi = under(a if kind == 0 else b)
            assert (box[:, 0] <= lo).all() and (box[:, 1] >= hi).all(), (what, "step", kind, box, lo, hi)
        return seen[0]

    for leaf_max in (1, 2, 4, 8):
        lay = rt.debug_ordered_layout(scene, walk=rt.RT_WALK_OWN_TREES, wide=0, leaf_max=leaf_max)
        assert lay["ordered"]
        two = lambda record: [(int(lay["nodes"][record][12 + k]), tol.f32_box(lay["nodes"][record][6 * k:6 * k + 6])) for k in range(2)]
        assert check_tree(lay, two, ("two children", leaf_max)) == n_moving
    for leaf_max in (1, 3, 8):
        opts = dict(walk=rt.RT_WALK_OWN_TREES, wide=1, leaf_max=leaf_max)
        lay, rec = rt.debug_ordered_layout(scene, **opts), rt.debug_wide_records(scene, **opts)
        assert lay["ordered"] and rec["wide"]
        four = lambda record: [(int(rec["refs"][record][k]), rec["boxes"][record][k].astype(np.float64)) for k in range(4)]
        assert check_tree(lay, four, ("four children", leaf_max)) == n_moving


def test_sphere_bounded_media_become_one_record(rt):
    _, nodes = nodes_of(rt, 8, True)            # final_scene: both media are bounded by a Sphere (src/main.rs:565-587)
    assert sum(nd.kind == NK_MEDIUM_SPHERE for nd in nodes) == 2 and not any(nd.kind == NK_MEDIUM_ENTER for nd in nodes)
    _, smoke = nodes_of(rt, 7, True)            # cornell_smoke: boundaries are Translate(RotateY(cube)) (src/main.rs:469-489)
    assert sum(nd.kind == NK_MEDIUM_ENTER for nd in smoke) == 2 and sum(nd.kind == NK_INST_ENTER for nd in smoke) == 2
