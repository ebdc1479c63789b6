"""rt_render_views_device / rt_render_views: many cameras of one scene in one launch (rt_kernel.hip path_kernel<..., JOBS_VIEWS>,
sum_view_samples_kernel).  Every view is held, as u64 views of its doubles, to the CPU oracle under that view's camera and seed
(oracle_lib.render(hs, params, camera=)): the views' tiles are stacked in one job space, so a wave's grab straddles views, and each
lane reads its own view's camera and seed.

Cameras come from camera_look (the host library's Camera::new over the scene's settings) unless a case edits fields in place.
An oracle frame is rendered once per (case, camera, seed, range) and shared between the tests that need it."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scene_cases
from adaptive_helpers import SENTINEL, assert_bits, bits, launches_for

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RT_ERR_INVALID_ARGUMENT, RT_ERR_UNSUPPORTED = -1, -5
C2, C3, C4 = "c2_random_balls_96x64_8spp_d50", "c3_cornell_box_64x64_16spp_d50", "c4_final_scene_64x64_8spp_d40"
RAGGED = "ragged_random_balls_53x29_4spp"

_scenes, _oracle_frames = {}, {}


def scene(rt, case):
    if case not in _scenes:
        _scenes[case] = scene_cases.build(rt, case)
    return _scenes[case]


# Cornell's box is open to the camera's side only and its background is black: from beside or behind it every frame is black, and
# two such views are the same frame.  Its views are therefore the first n of a 30-view orbit, 12 degrees apart: all look inside.
CORNELL_ARC = 30


def orbit(rt, hs, n, seed0, of=None):
    """n views: view 0 the scene's own camera, view k looking from the k-th point of the orbit (of `of` points, if given);
    distinct seeds"""
    views = rt.orbit_views(hs, n, seed0, of)
    assert bytes(views[0].camera) == bytes(hs.camera)
    assert len({views[k].seed for k in range(n)}) == n
    return views


def oracle_frame(rt, oracle, case, view, **range_kw):
    """the oracle's frame under exactly this view's camera and seed (cached: keyed by the camera's bytes)"""
    key = (case, bytes(view.camera), int(view.seed), tuple(sorted(range_kw.items())))
    if key not in _oracle_frames:
        cam = rt.Camera.from_buffer_copy(bytes(view.camera))
        frame = oracle.render(scene(rt, case), rt.render_params(seed=int(view.seed), **range_kw), camera=cam)
        frame.setflags(write=False)
        _oracle_frames[key] = frame
    return _oracle_frames[key]


def assert_views_equal_oracle(rt, oracle, case, views, got, what, **range_kw):
    n = len(views)
    got = np.asarray(got).reshape(n, -1)
    for v in range(n):
        assert_bits(got[v], oracle_frame(rt, oracle, case, views[v], **range_kw), f"{what}: view {v} of {n}")


def render_on_device(ds, rt, views, params, extra=0, fill=None):
    """rt_render_views_device into a torch buffer of n frames (+ `extra` doubles behind them), pre-filled with the sentinel"""
    import torch
    n = len(views)
    frame = views[0].camera.image_width * views[0].camera.image_height * 3
    d = torch.full((n * frame + extra,), int(SENTINEL) if fill is None else fill, dtype=torch.int64, device="cuda").view(torch.float64)
    ds.render_views_device(params, views, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    return out[:n * frame].reshape(n, frame), out[n * frame:]


@pytest.mark.parametrize("case, n_views", [(C2, 5), (C3, 5), (C4, 3)])
def test_each_view_equals_the_oracle(rt, oracle, gpu, case, n_views):
    hs = scene(rt, case)
    views = orbit(rt, hs, n_views, 11, CORNELL_ARC if case == C3 else None)
    got = rt.DeviceScene(hs).render_views(rt.render_params(seed=999), views)  # (params.seed is ignored)
    assert got.shape == (n_views, hs.height, hs.width, 3)
    assert_views_equal_oracle(rt, oracle, case, views, got, case)
    assert rt.debug_last_launch()["launches"] == 1
    frames = {bits(got[v]).tobytes() for v in range(n_views)}
    assert len(frames) == n_views, "two views rendered the same frame"


def test_view_boundaries_inside_a_waves_grab(rt, oracle, gpu):
    """53x29: 7 x 4 = 28 tiles per view with padding pixels on two edges; 4 spp make a view 28 * 4 * 64 = 7168 jobs, no multiple
    of any grab size's share of a tile row: 128-job grabs straddle tiles and views.  The doubles behind the last view stay untouched."""
    hs = scene(rt, RAGGED)
    assert (hs.width, hs.height) == (53, 29)
    views = orbit(rt, hs, 7, 21)
    got, tail = render_on_device(rt.DeviceScene(hs), rt, views, rt.render_params(), extra=1024)
    assert_views_equal_oracle(rt, oracle, RAGGED, views, got, RAGGED)
    assert (bits(tail) == SENTINEL).all(), "the buffer behind the last view was written"


def test_a_view_without_defocus_between_two_with(rt, oracle, gpu):
    """random-balls has defocus_angle 0.6: the view in the middle has 0, so lanes of one wave take both sides of the disk loop and
    draw different numbers of values"""
    hs = scene(rt, C2)
    views = orbit(rt, hs, 3, 31)
    assert views[0].camera.defocus_angle == 0.6
    views[1].camera.defocus_angle = 0.0
    got = rt.DeviceScene(hs).render_views(rt.render_params(), views)
    assert_views_equal_oracle(rt, oracle, C2, views, got, "defocus 0.6 / 0 / 0.6")


def test_a_view_with_its_own_background(rt, oracle, gpu):
    """Cornell's background is black: one view's is (0.1, 0.2, 0.3), the views beside it keep the scene's"""
    hs = scene(rt, C3)
    views = orbit(rt, hs, 3, 41)
    # (from outside the box nearly every path ends on the background; view 1 looks at the box's side wall from there)
    assert views[0].camera.background.tuple() == (0.0, 0.0, 0.0)
    views[1].camera.background.x, views[1].camera.background.y, views[1].camera.background.z = 0.1, 0.2, 0.3
    got = rt.DeviceScene(hs).render_views(rt.render_params(), views)
    assert_views_equal_oracle(rt, oracle, C3, views, got, "background black / (0.1, 0.2, 0.3) / black")
    plain = oracle_frame(rt, oracle, C3, orbit(rt, hs, 3, 41)[1])
    assert (bits(got[1].reshape(-1)) != bits(plain)).any(), "the view's own background changed nothing: the case checks nothing"


@pytest.mark.parametrize("case", [C2, C3])
def test_same_frames_on_every_walk(rt, oracle, gpu, case):
    hs = scene(rt, case)
    views = list(orbit(rt, hs, 5, 11, CORNELL_ARC if case == C3 else None))[:3]  # (the first test's views: their oracle frames are shared)
    frames = {}
    for name, opts in (("reference order", dict(walk=rt.RT_WALK_REFERENCE_ORDER)), ("own trees, two children", dict(walk=rt.RT_WALK_OWN_TREES, wide=0)),
                       ("own trees, four children", dict(walk=rt.RT_WALK_OWN_TREES, wide=1))):
        frames[name] = rt.DeviceScene(hs, **opts).render_views(rt.render_params(), views)
    first = frames["reference order"]
    assert_views_equal_oracle(rt, oracle, case, views, first, f"{case} reference order")
    for name, f in frames.items():
        assert_bits(f, first, f"{case}: {name} against the reference order")


def test_sample_ranges_accumulate(rt, oracle, gpu):
    hs = scene(rt, C2)
    views = list(orbit(rt, hs, 5, 11))[:3]
    assert hs.camera.samples_per_pixel == 8
    ds = rt.DeviceScene(hs)
    whole = ds.render_views(rt.render_params(sample_begin=0, sample_end=8), views)
    import torch
    frame = hs.width * hs.height * 3
    d = torch.zeros(3 * frame, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ds.render_views_device(rt.render_params(sample_begin=0, sample_end=3), views, d.data_ptr(), stream)
    ds.render_views_device(rt.render_params(sample_begin=3, sample_end=8, accumulate=True), views, d.data_ptr(), stream)
    torch.cuda.synchronize()
    split = d.cpu().numpy().reshape(3, frame)
    assert_bits(split, whole.reshape(3, frame), "[0, 3) + [3, 8) against [0, 8)")
    assert_views_equal_oracle(rt, oracle, C2, views, whole, "[0, 8)")


CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import scene_cases
rt = importlib.import_module("rust-tracing_amd")
case, out, n_views, seed0, spp, of = sys.argv[2], sys.argv[3], *map(int, sys.argv[4:8])
hs = scene_cases.build(rt, case)
views = rt.orbit_views(hs, n_views, seed0, of)
got = rt.DeviceScene(hs).render_views(rt.render_params(sample_end=spp), views)
np.save(out + ".npy", got)
print(json.dumps({"launches": rt.debug_last_launch()["launches"]}))
"""


@pytest.mark.parametrize("overlap", [0, 1])
def test_a_views_render_of_several_launches(rt, oracle, gpu, tmp_path, overlap):
    """5 views of Cornell 64x64 at 9 spp under a 1 MiB sample buffer: a sample row is 5 * 64 tiles * 64 * 24 B = 480 KiB.  The child
    renders; the parent holds its launch count to the chunk arithmetic and its frames to the oracle, which the child never loads."""
    n_views, spp, seed0, budget = 5, 9, 71, 1 << 20
    hs = scene(rt, C3)
    entries = n_views * 64 * 64
    assert entries * 24 == 480 * 1024
    want_launches = launches_for(entries, spp, budget, overlap)[0]
    assert want_launches >= 3
    out = str(tmp_path / "child")
    env = dict(os.environ, RT_SAMPLE_BUFFER_MB="1", RT_OVERLAP=str(overlap))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), C3, out, str(n_views), str(seed0), str(spp), str(CORNELL_ARC)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["launches"] == want_launches, (stats, want_launches)
    views = orbit(rt, hs, n_views, seed0, CORNELL_ARC)
    assert_views_equal_oracle(rt, oracle, C3, views, np.load(out + ".npy"), f"several launches, RT_OVERLAP={overlap}", sample_end=spp)


def test_one_view_equals_rt_render_device(rt, oracle, gpu):
    import torch
    hs = scene(rt, C2)
    ds = rt.DeviceScene(hs)
    view = orbit(rt, hs, 5, 11)[1]
    cam = rt.Camera.from_buffer_copy(bytes(view.camera))
    frame = hs.width * hs.height * 3
    d = torch.zeros(frame, dtype=torch.float64, device="cuda")
    ds.render_device(rt.render_params(seed=int(view.seed)), d.data_ptr(), torch.cuda.current_stream().cuda_stream, camera=cam)
    torch.cuda.synchronize()
    got, _ = render_on_device(ds, rt, [view], rt.render_params(seed=5))
    assert_bits(got[0], d.cpu().numpy(), "one view against rt_render_device")
    assert_bits(got[0], oracle_frame(rt, oracle, C2, view), "one view against the oracle")


def test_refusals(rt, gpu):
    """Each refused call returns its status with a message that names the field, launches nothing and leaves d_out as it was"""
    import torch
    hs = scene(rt, C2)
    ds = rt.DeviceScene(hs)
    lib = rt.amd_lib()
    frame = hs.width * hs.height * 3
    stream = torch.cuda.current_stream().cuda_stream
    d = torch.full((2 * frame,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)

    def call(views, n, params):
        ds.render_device(rt.render_params(sample_end=1), torch.zeros(frame, dtype=torch.float64, device="cuda").data_ptr(), stream)
        assert rt.debug_last_launch()["launches"] == 1
        rc = lib.rt_render_views_device(ds._handle, views, n, C.byref(params), C.c_void_p(d.data_ptr()), C.c_void_p(stream))
        msg = lib.rt_last_error().decode()
        torch.cuda.synchronize()
        assert (d.cpu().numpy().view(np.uint64) == SENTINEL).all(), f"a refused call wrote to d_out ({msg})"
        assert rt.debug_last_launch()["launches"] == 0, f"a refused call launched ({msg})"
        return rc, msg

    def two():
        return rt.orbit_views(hs, 2, 1)

    views = two()
    views[1].camera.image_width += 8
    rc, msg = call(views, 2, rt.render_params())
    assert rc == RT_ERR_INVALID_ARGUMENT and "image_width" in msg and "views[1]" in msg, (rc, msg)

    rc, msg = call(two(), 0, rt.render_params())
    assert rc == RT_ERR_INVALID_ARGUMENT and "n_views" in msg, (rc, msg)

    rc, msg = call(two(), 2, rt.render_params(shard_count=2))
    assert rc == RT_ERR_INVALID_ARGUMENT and "shard_count" in msg, (rc, msg)

    rc, msg = call(two(), 2, rt.render_params(out_layout=rt.RT_OUT_TILES))
    assert rc == RT_ERR_INVALID_ARGUMENT and "out_layout" in msg, (rc, msg)

    views = two()
    views[1].camera.samples_per_pixel += 1
    rc, msg = call(views, 2, rt.render_params(sample_end=0))
    assert rc == RT_ERR_INVALID_ARGUMENT and "samples_per_pixel" in msg, (rc, msg)
    # ... which params->sample_end settles
    rc = lib.rt_render_views_device(ds._handle, views, 2, C.byref(rt.render_params(sample_end=2)), C.c_void_p(d.data_ptr()), C.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == 0 and not (d.cpu().numpy().view(np.uint64) == SENTINEL).any()
    d.view(torch.int64).fill_(int(SENTINEL))

    # 2^26 views of an 8x8 frame (one tile each): more tiles than the job index holds.  Refused before d_out (one frame) or the
    # views beyond the first are looked at.
    tiny = scene_cases.build(rt, C2, width=8, aspect=1.0)
    assert (tiny.width, tiny.height) == (8, 8)
    one = rt.orbit_views(tiny, 1, 1)
    ds8 = rt.DeviceScene(tiny)
    d8 = torch.full((8 * 8 * 3,), int(SENTINEL), dtype=torch.int64, device="cuda").view(torch.float64)
    rc = lib.rt_render_views_device(ds8._handle, one, 1 << 26, C.byref(rt.render_params()), C.c_void_p(d8.data_ptr()), C.c_void_p(stream))
    msg = lib.rt_last_error().decode()
    torch.cuda.synchronize()
    assert rc == RT_ERR_UNSUPPORTED and "n_views" in msg, (rc, msg)
    assert (d8.cpu().numpy().view(np.uint64) == SENTINEL).all() and rt.debug_last_launch()["launches"] == 0
